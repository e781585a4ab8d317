"""fp64 references, derived worst-case error bounds, case lists and f32 CPU emulations of the HBM-bound glue kernels of the ViT
trainer (a helper module, like attn_bwd_reference.py; test_vit_glue_reference_cpu.py proves the gate on the CPU,
test_gpu_vit_glue.py applies it to the kernels): the column sums, LayerNorm forward and backward, the wrapper head's backward,
the loss, and the exact kernels token_reduce / cls_rows / sgd_step.

Every reference is a function of the OPERANDS the kernel is given.  The gate is |got - ref| <= GATE * B for EVERY element,
GATE = 1.01, with B a worst-case bound built from two constants only: EPS = 2^-24, one f32 rounding, and U = 2^-8, the unit roundoff
of round-to-nearest bf16.  The 1 % is for second-order terms.  Nothing is fitted.  The library is built with -ffp-contract=off and
correctly rounded division and square root, so every f32 operation below is one rounding of at most EPS relative; expf, logf and
log1pf are given 2 EPS (one ulp).

Two rules carry every derivation:
  (S) a sum whose every term passes through at most d additions is off by at most d * EPS * sum|x_i| (each addition rounds a
      partial sum, which is at most the sum of the |x_i| it holds; a term is charged once per addition on its path).  d is read off
      the kernel: it never exceeds the number of terms, so this is the `n * EPS * sum|x_i|` rule with the kernel's own tree depth.
  (P) a product of factors known to +-d_i is off by at most prod(|f_i| + d_i) - prod|f_i| (not linearised: it stays a bound where
      a factor is smaller than its own error, as 1 - exp(-bce) is in the focal term), plus EPS of the result per multiplication.

Column sums (csrc/vit_bwd.hip).  A workgroup of cast_colsum_kernel (lines 43-57), colsum_bf16_kernel (59-68), colsum_bf16_vec_kernel
(73-109: 8 row lanes, 4 rows per lane, lanes added in order, lines 104-106) or cast_colsum_vec_kernel (111-146: 4 row lanes, 8 rows
per lane) sums CS_ROWS = 32 rows: at most 32 additions on a term's path whichever kernel runs.  reduce_rows_kernel (148-188) adds
every 32nd partial row per group and then the 32 groups in order, reduce_rows_scalar_kernel (192-211) every 8th and 8 groups:
    red_depth(parts) = max(ceil(parts / 32) + 32, ceil(parts / 8) + 8)
    B_colsum = (32 + red_depth(parts) + [accumulate]) * EPS * (sum_r |x_rc| + |start_c|)
The bf16 copy y of yv_cast_colsum is exact: RNE of x bit for bit (pack_bf16x2 / f32_to_bf16).

LayerNorm forward (csrc/vit_misc.hip, layernorm_kernel).  Lane l adds its float4 chunks l, l + 64, ... as (x + y) + (z + w) (line
38: 2 + ceil(D / 256) additions), wave_sum adds 6 more (yv_common.h:65-69): d = ceil(D / 256) + 8.
    d_mean = (d + 1) EPS mean|x|                       (line 41: the sum and the division)
    d_a    = d_mean + EPS |a|                          a = x - mean (line 47)
    d_var  = (sum((|a| + d_a)^2 - a^2) + (d + 1) EPS sum a^2) / D + 2 EPS (var + eps)        (lines 48, 51: products, sum, / D, + eps)
    r      = d_var / (2 (var + eps)) + 4 EPS           relative error of rstd (line 51: sqrtf, 1 / x)
    E      = |gamma| rstd d_a + |a rstd gamma| (r + 2 EPS) + EPS |y|                          (line 58: two products, one addition)
    B_y    = U |y| + E                                 (line 60: pack_bf16x2, RNE of the f32 value)

LayerNorm backward (csrc/vit_bwd.hip, layernorm_bwd_kernel, lines 226-311; the statistics as above, lines 257-270), g = dy:
    d_xhat = rstd d_a + |xhat| (r + EPS)               (line 276)
    gg = g gamma (line 279, EPS |gg|);  m1 = sum gg / D,  m2 = sum gg xhat / D  (lines 280-284):
    d_m1 = (d + 2) EPS mean|gg|      d_m2 = (sum |gg| d_xhat + (d + 3) EPS sum |gg xhat|) / D
    t = gg - m1 - xhat m2 (line 291):  d_t = EPS |gg| + d_m1 + ((|xhat| + d_xhat)(|m2| + d_m2) - |xhat m2|) + EPS |xhat m2|
                                             + 2 EPS (|gg| + |m1| + |xhat m2|)
    B_dx = rstd d_t + |rstd t| (r + EPS) + EPS |dx0 + LN'|     (lines 291-293: the product and the read-modify-write addition)
    dgamma_c = sum_r g xhat, dbeta_c = sum_r g: a lane adds its workgroup's LNB_ROWS / 4 = 2 rows (lines 277-278), the four waves
    are added as a tree (lines 308-309: 2), then launch_reduce_rows over the ceil(rows / 8) partial rows:
    B_dgamma = sum_r |g| d_xhat + (5 + red_depth(blocks)) EPS sum_r |g xhat|      (one more for the product)
    B_dbeta  = (4 + red_depth(blocks)) EPS sum_r |g|

Wrapper-head backward (csrc/vit_bwd.hip, head_bwd_a_kernel 327-348, head_bwd_b_kernel 351-389; fmaf chains, f = relu(feats)):
    h = relu(sum_k f_k W1[u,k] + b1_u): two chains of 500 (line 338), two additions (342):   d_h = 503 EPS (sum |f W1| + |b1|)
    dh = (sum_c dl_c W2[c,u]) [h > 0] (line 344):                                            d_dh = (nc + 1) EPS sum |dl W2|
    dW1[u,k] = sum_r dh f (362): sum_r d_dh f + (R + 1) EPS sum |dh f|        db1 = sum_r dh (375): sum_r d_dh + R EPS sum |dh|
    dW2[c,u] = sum_r dl h (380): sum_r |dl| d_h + (R + 1) EPS sum |dl h|      db2 = sum_r dl (385): R EPS sum |dl|
    dfeats[r,k] = bf16(sum_u dh W1[u,k]) [feats > 0] (368-370): U |ref| + sum_u d_dh |W1| + 129 EPS sum |dh W1|
    The two ReLU decisions are discontinuous: head_case builds inputs whose pre-activations and non-zero features are, in fp64, at
    least RELU_MARGIN from zero, and asserts that and d_h < RELU_MARGIN: no decision can differ in f32 and no element is left out.

Loss (csrc/train.hip, loss_kernel, lines 14-50), z = x - max x, e = expf(z), p = e / den, t = one-hot, on logits within
+-LOGIT_RANGE (the f32 form of the reference itself is finite at +-40 and infinite at +-80, where -log(softmax) underflows):
    rel_e = EPS |z| + 2 EPS (line 26)   rel_den = max_c rel_e + nc EPS   d_p = p (rel_e + rel_den + EPS) (line 29)
    g_ls = (p - 0.9 t - 0.1 / nc) / B (line 40): d = (d_p + 3 EPS (p + 0.9 t + 0.1 / nc) + 2 EPS |p - ..|) / B
    bce = max(x, 0) - x t + log1pf(expf(-|x|)) (line 35: non-negative terms): d_bce = 8 EPS bce
    pt = expf(-bce) (36): d_pt = pt (d_bce + 2 EPS)     om = 1 - pt (37): d_om = d_pt + EPS om
    s = sigmoid(x) - t (39, 41): d_s = 5 EPS sigmoid + EPS |s|
    g_fo = s om (2 pt bce + om) / (B nc) (line 41): rule (P) on the three factors, + 5 EPS of the result
    B_grad = w_ls d(g_ls) + w_fo d(g_fo) + 2 EPS (|w_ls g_ls| + |w_fo g_fo|) + EPS |grad|        (line 42; the weights are f32)
    nl = -logf(p) (30): d_nl = d_p / p + 2 EPS |nl|;  a row's value (line 44) v = (0.9 cross + 0.1 smooth / nc) / B w_ls
    + sum_c om^2 bce / (B nc) w_fo with rule (P) on om^2 bce and rule (S) over the classes; a thread adds ceil(B / 256) rows (line
    20), wave_sum 6, line 49 adds 3:
    B_loss = sum_rows d_v + (ceil(B / 256) + 9) EPS sum_rows v
    Rule (P) keeps the focal term bounded where 1 - expf(-bce) cancels to zero in f32 (bce ~ 1e-13 at |x| = 30): the error of
    om^2 bce is then d_om^2 bce = 4 EPS^2 bce, below the EPS * bce a linearised bound would need as an absolute floor.

Exact: token_reduce, cls_rows, the integer cases of every column sum and of dbeta (bf16-representable integers in [-8, 8], sums
below 2^24: every partial sum is an integer f32 holds), and sgd_step (oracle.train.sgd_step evaluated in f32, one rounding per
operation, is the kernel's __f*_rn sequence, train.hip:63-65).
"""
import functools

import torch

from oracle import train as ot

U = 2.0 ** -8                      # unit roundoff of round-to-nearest bf16
EPS = 2.0 ** -24                   # unit roundoff of f32
GATE = 1.01                        # derived (second-order terms), not fitted
CS_ROWS = 32                       # rows per workgroup of the column-sum kernels
LNB_ROWS = 8                       # rows per workgroup of layernorm_bwd_kernel
RELU_MARGIN = 1e-3
LOGIT_RANGE = 30.0
LN_EPS = 1e-6
NAN_ROWS = 2                       # input rows past `rows`, all NaN


def bf(t):
    return t.to(torch.bfloat16)


def worst(got, ref, bound):
    """-> (max |got - ref| / bound, flat index of it); 0 / 0 counts as 0, anything non-finite or x / 0 as inf."""
    diff = (got.double() - ref).abs().reshape(-1)
    b = bound.reshape(-1)
    ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / b)
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    i = int(ratio.argmax())
    return float(ratio[i]), i


def red_depth(parts):
    """additions on a term's path through launch_reduce_rows, whichever of its two kernels runs"""
    return max((parts + 31) // 32 + 32, (parts + 7) // 8 + 8)


def int_tensor(shape, gen, lo=-8, hi=8):
    """bf16-representable integers in [lo, hi] as f32"""
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


# ------------------------------------------------------------------------------------------------ ordered f32 sums
def lane_chain(x, L):
    """x (..., n, cols) f32 -> (..., cols): lane l of L adds rows l, l + L, ... in order, then the lanes are added in lane order
    (the shape of every two-stage sum in vit_bwd.hip; a lane without rows holds 0)."""
    n, cols = x.shape[-2], x.shape[-1]
    k = (n + L - 1) // L
    xp = torch.cat([x, torch.zeros(*x.shape[:-2], k * L - n, cols, dtype=x.dtype)], -2).reshape(*x.shape[:-2], k, L, cols)
    s = xp[..., 0, :, :].clone()
    for j in range(1, k):
        s = s + xp[..., j, :, :]
    t = s[..., 0, :].clone()
    for l in range(1, L):
        t = t + s[..., l, :]
    return t


# ------------------------------------------------------------------------------------------------ column sums
def colsum_path(kind, cols, ld=None, aligned=True):
    """-> (row lanes of the first stage, row groups of the second): the routing of yv_cast_colsum / yv_colsum_bf16 (vit_bwd.hip
    C ABI) and launch_reduce_rows for a 16-byte aligned workspace."""
    if kind == "cast":
        L = 4 if cols % 4 == 0 and aligned else 1
    else:
        L = 8 if cols % 8 == 0 and (cols if ld is None else ld) % 8 == 0 else 1
    return L, (32 if cols % 4 == 0 else 8)


def colsum_reference(x, start=None):
    """x (rows, cols), optional start (cols) for accumulate -> (ref, bound) in fp64 (module docstring)."""
    x64 = x.double()
    parts = (x.shape[0] + CS_ROWS - 1) // CS_ROWS
    ref, mass, depth = x64.sum(0), x64.abs().sum(0), CS_ROWS + red_depth(parts)
    if start is not None:
        ref, mass, depth = ref + start.double(), mass + start.double().abs(), depth + 1
    return ref, depth * EPS * mass


COLSUM_MUTANTS = ("drop_block_last_row", "drop_lane_tail", "ignore_accumulate")


def emu_colsum(x, L, G, start=None, mutant=None):
    """f32 emulation of a column-sum kernel with L row lanes followed by the second stage with G row groups."""
    x = x.float().clone()
    rows, cols = x.shape
    if mutant == "drop_block_last_row":                      # r1 = min(rows, r0 + rows_per_block - 1)
        x[CS_ROWS - 1::CS_ROWS] = 0
    if mutant == "drop_lane_tail":                           # only whole trips of 4 rows per lane: the `rr < r1` tail is never loaded
        r0 = (rows - 1) // CS_ROWS * CS_ROWS
        x[r0 + (rows - r0) // (4 * L) * (4 * L):] = 0
    parts = (rows + CS_ROWS - 1) // CS_ROWS
    xb = torch.cat([x, torch.zeros(parts * CS_ROWS - rows, cols)]).reshape(parts, CS_ROWS, cols)
    out = lane_chain(lane_chain(xb, L), G)
    if start is not None and mutant != "ignore_accumulate":
        out = start.float() + out
    return out


# (kind, rows, cols): the shapes of test_gpu_vit_glue.py that the CPU proof walks too
COLSUM_CASES = [("cast", r, c) for c in (4, 260, 300, 768, 5, 37) for r in (1, 31, 32, 33, 47)] + [("cast", 4131, 8), ("cast", 4131, 5)] + \
               [("bf16", r, c) for c in (8, 264, 300) for r in (1, 31, 33, 47)] + [("bf16", 9, 1024), ("bf16", 70, 3072), ("bf16", 4131, 8)]


@functools.lru_cache(maxsize=None)
def colsum_case(kind, rows, cols, exact=False):
    """-> dict: x (rows, cols) f32 (bf16-representable for kind bf16), start (cols).  exact: integers in [-8, 8]."""
    g = torch.Generator().manual_seed((rows * 4099 + cols) * 4 + (kind == "bf16") * 2 + exact)
    if exact:
        return {"x": int_tensor((rows, cols), g), "start": int_tensor((cols,), g, -100, 100)}
    x = torch.randn(rows, cols, generator=g) * 2 + 0.25
    return {"x": bf(x).float() if kind == "bf16" else x, "start": torch.randn(cols, generator=g) * 3}


def rne_bits_case(rows, cols):
    """f32 whose bf16 rounding is decided at every kind of boundary: random bit patterns, exact ties above an even and an odd
    mantissa, one f32 ulp either side of a tie, +-0, +-inf, the largest finite f32 (rounds to inf), denormals."""
    g = torch.Generator().manual_seed(rows * 131 + cols)
    n = rows * cols
    hi = torch.randint(0, 1 << 16, (n,), generator=g, dtype=torch.int64)
    hi = torch.where((hi & 0x7f80) == 0x7f80, hi & 0x807f | 0x3f80, hi)                 # no NaN / inf from the random part
    lo = torch.randint(0, 1 << 16, (n,), generator=g, dtype=torch.int64)
    sel = torch.arange(n) % 4
    lo = torch.where(sel == 1, torch.full_like(lo, 0x8000), lo)                          # exact ties
    lo = torch.where(sel == 2, 0x8000 + (torch.arange(n) % 3 - 1), lo)                   # a tie and its two f32 neighbours
    bits = (hi << 16) | lo
    special = torch.tensor([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7f7fffff, 0xff7fffff, 0x00000001, 0x80008000,
                            0x3f808000, 0x3f818000, 0x7f7f8000])
    bits[:special.numel()] = special[:n]
    bits = torch.where(bits >= 1 << 31, bits - (1 << 32), bits).to(torch.int32)
    return bits.view(torch.float32).reshape(rows, cols)


# ------------------------------------------------------------------------------------------------ LayerNorm
LN_DS = (4, 192, 260, 768, 1024)
LN_FWD_CASES = [(D, r, "plain") for D in LN_DS for r in (1, 3, 4, 5, 70)] + [(192, 5, "strided"), (1024, 5, "strided"), (128, 9, "lowvar")]
LN_BWD_CASES = [(D, r, "plain") for D in LN_DS for r in (1, 7, 8, 9, 70)] + [(128, 1037, "plain"), (192, 9, "strided"),
                                                                             (1024, 9, "strided"), (128, 9, "lowvar")]
LN_MUTANTS_FWD = ("eps_1e-5", "var_over_d_minus_1", "gamma_chunk_shift", "ignore_ldx")
LN_MUTANTS_BWD = ("eps_1e-5", "var_over_d_minus_1", "gamma_chunk_shift", "drop_m2", "dgamma_from_g_gamma", "ignore_ldx", "ignore_lddy")


def _strided(live, ld, fill, extra_rows):
    """live (rows, D) -> buffer (rows + extra_rows, ld) holding it in its first D columns, `fill` everywhere else"""
    rows, D = live.shape
    buf = torch.full((rows + extra_rows, ld), fill, dtype=live.dtype)
    buf[:rows, :D] = live
    return buf


@functools.lru_cache(maxsize=None)
def ln_case(D, rows, kind):
    """The operands of one LayerNorm case, forward and backward, on the CPU; read-only by agreement.
    plain: every stride D; strided: ldx = lddx = 3 D, ldy = lddy = D + 4 (the final norm over the cls rows has ldx = lddx = N D);
    lowvar: row std 0.01 around 0.5 (var 1e-4: the only data on which eps 1e-5 for 1e-6 shows).
    -> dict: x, gamma, beta, dy (bf16), dx0 (rows, D); xbuf / dybuf: the strided buffers with NaN in every gap and in NAN_ROWS rows
    past `rows`; ldx, ldy."""
    g = torch.Generator().manual_seed((D * 2053 + rows) * 3 + ("plain", "strided", "lowvar").index(kind))
    x = 0.5 + 0.01 * torch.randn(rows, D, generator=g) if kind == "lowvar" else torch.randn(rows, D, generator=g) * 2 + 0.3
    c = {"D": D, "rows": rows, "kind": kind, "x": x,
         "gamma": 1 + 0.1 * torch.randn(D, generator=g), "beta": 0.1 * torch.randn(D, generator=g),
         "dy": bf(torch.randn(rows, D, generator=g)), "dx0": torch.randn(rows, D, generator=g),
         "ldx": 3 * D if kind == "strided" else D, "ldy": D + 4 if kind == "strided" else D}
    c["xbuf"] = _strided(x, c["ldx"], float("nan"), NAN_ROWS)
    c["dybuf"] = _strided(c["dy"], c["ldy"], float("nan"), NAN_ROWS)
    return c


def _ln_depth(D):
    return (D + 255) // 256 + 8


def _ln_stats64(x, D, eps):
    """-> mean-free a, rstd, and the error terms d_a (absolute) and r (relative, of rstd) of the module docstring"""
    d = _ln_depth(D)
    mean = x.mean(-1, keepdim=True)
    a = x - mean
    var = (a * a).mean(-1, keepdim=True)
    d_a = (d + 1) * EPS * x.abs().mean(-1, keepdim=True) + EPS * a.abs()
    d_var = (((a.abs() + d_a) ** 2 - a * a).sum(-1, keepdim=True) + (d + 1) * EPS * (a * a).sum(-1, keepdim=True)) / D + 2 * EPS * (var + eps)
    return a, 1.0 / torch.sqrt(var + eps), d_a, d_var / (2 * (var + eps)) + 4 * EPS


def ln_fwd_reference(x, gamma, beta, eps=LN_EPS):
    """x (rows, D), gamma, beta (D) -> (y, B_y) in fp64."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    a, rstd, d_a, r = _ln_stats64(x, x.shape[1], eps)
    y = a * rstd * gamma + beta
    return y, U * y.abs() + gamma.abs() * rstd * d_a + (a * rstd * gamma).abs() * (r + 2 * EPS) + EPS * y.abs()


def ln_bwd_reference(x, gamma, dy, dx0, eps=LN_EPS):
    """-> dict: dx (= dx0 + LN'(dy), fp64), dgamma, dbeta and the bounds b_dx, b_dgamma, b_dbeta."""
    x, gamma, g, dx0 = x.double(), gamma.double(), dy.double(), dx0.double()
    rows, D = x.shape
    d = _ln_depth(D)
    a, rstd, d_a, r = _ln_stats64(x, D, eps)
    xhat = a * rstd
    d_xhat = rstd * d_a + xhat.abs() * (r + EPS)
    gg = g * gamma
    m1, m2 = gg.mean(-1, keepdim=True), (gg * xhat).mean(-1, keepdim=True)
    d_m1 = (d + 2) * EPS * gg.abs().mean(-1, keepdim=True)
    d_m2 = ((gg.abs() * d_xhat).sum(-1, keepdim=True) + (d + 3) * EPS * (gg * xhat).abs().sum(-1, keepdim=True)) / D
    t = gg - m1 - xhat * m2
    xm = (xhat * m2).abs()
    d_t = EPS * gg.abs() + d_m1 + ((xhat.abs() + d_xhat) * (m2.abs() + d_m2) - xm) + EPS * xm + 2 * EPS * (gg.abs() + m1.abs() + xm)
    dx = dx0 + rstd * t
    depth = red_depth((rows + LNB_ROWS - 1) // LNB_ROWS)
    return {"dx": dx, "b_dx": rstd * d_t + (rstd * t).abs() * (r + EPS) + EPS * dx.abs(),
            "dgamma": (g * xhat).sum(0), "b_dgamma": (g.abs() * d_xhat).sum(0) + (5 + depth) * EPS * (g * xhat).abs().sum(0),
            "dbeta": g.sum(0), "b_dbeta": (4 + depth) * EPS * g.abs().sum(0)}


def _rows_of(buf, rows, D, ld):
    """the (rows, D) operand a kernel reads from `buf` with row stride ld"""
    return buf.reshape(-1).as_strided((rows, D), (ld, 1))


def _lanes(x, D):
    """(rows, D) f32 -> (rows, 4, 64, 4), zero padded: [i][lane][xyzw] is float4 chunk lane + 64 i of the row"""
    xp = torch.zeros(x.shape[0], 1024)
    xp[:, :D] = x
    return xp.view(-1, 4, 64, 4)


def _lane_sum(v):
    """layernorm_kernel's per-lane sum over its chunks, each as (x + y) + (z + w), then wave_sum's xor butterfly -> (rows, 1, 1, 1)"""
    s = torch.zeros(v.shape[0], 64)
    for i in range(4):
        s = s + ((v[:, i, :, 0] + v[:, i, :, 1]) + (v[:, i, :, 2] + v[:, i, :, 3]))
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, idx ^ o]
    return s[:, 0].reshape(-1, 1, 1, 1)


def _emu_stats(x, D, eps, mutant):
    live = (_lanes(torch.ones(1, D), D) > 0)
    v = _lanes(x, D)
    fD = torch.tensor(float(D), dtype=torch.float32)
    a = (v - _lane_sum(v) / fD) * live
    var = _lane_sum(a * a) / (fD - 1 if mutant == "var_over_d_minus_1" else fD)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(1e-5 if mutant == "eps_1e-5" else eps, dtype=torch.float32))
    return a, rstd, live


def _gamma(gamma, mutant):
    return torch.roll(gamma, -4) if mutant == "gamma_chunk_shift" else gamma


def emu_ln_fwd(c, mutant=None, eps=LN_EPS):
    """f32 emulation of layernorm_kernel in its own operation order on the buffers of ln_case -> y (rows, D) bf16."""
    D, rows = c["D"], c["rows"]
    x = _rows_of(c["xbuf"], rows, D, D if mutant == "ignore_ldx" else c["ldx"])
    a, rstd, _ = _emu_stats(x, D, eps, mutant)
    o = a * rstd * _lanes(_gamma(c["gamma"], mutant)[None], D) + _lanes(c["beta"][None], D)
    return bf(o.reshape(rows, 1024)[:, :D])


def emu_ln_bwd(c, mutant=None, G=32, eps=LN_EPS):
    """f32 emulation of layernorm_bwd_kernel + the second stage with G row groups -> dx, dgamma, dbeta (f32)."""
    D, rows = c["D"], c["rows"]
    x = _rows_of(c["xbuf"], rows, D, D if mutant == "ignore_ldx" else c["ldx"])
    dy = _rows_of(c["dybuf"], rows, D, D if mutant == "ignore_lddy" else c["ldy"]).float()
    a, rstd, live = _emu_stats(x, D, eps, mutant)
    fD = torch.tensor(float(D), dtype=torch.float32)
    xhat = a * rstd
    g = _lanes(dy, D)
    gg = g * _lanes(_gamma(c["gamma"], mutant)[None], D)
    m1, m2 = _lane_sum(gg) / fD, _lane_sum(gg * xhat) / fD
    t = gg - m1 if mutant == "drop_m2" else gg - m1 - xhat * m2
    dx = _lanes(c["dx0"], D) + rstd * t

    def columns(term):                                      # two rows per wave, (w0 + w1) + (w2 + w3), then the second stage
        term = (term * live).reshape(rows, 1024)[:, :D]
        blocks = (rows + LNB_ROWS - 1) // LNB_ROWS
        tb = torch.cat([term, torch.zeros(blocks * LNB_ROWS - rows, D)]).reshape(blocks, 4, 2, D)
        w = tb[:, :, 0] + tb[:, :, 1]
        return lane_chain((w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3]), G)
    return dx.reshape(rows, 1024)[:, :D], columns((gg if mutant == "dgamma_from_g_gamma" else g) * xhat), columns(g)


# ------------------------------------------------------------------------------------------------ wrapper-head backward
HEAD_CASES = [(1, 1, 1000, 1000), (9, 5, 1024, 1024), (70, 32, 1000, 1024)]       # R, nc, ldf, ldd
HB_FEAT, HB_HID = 1000, 128


@functools.lru_cache(maxsize=None)
def head_case(R, nc, ldf, ldd):
    """Operands of yv_head_bwd with every ReLU decision RELU_MARGIN clear of zero in fp64 (asserted): features below 0.05 in
    magnitude are set to exactly 0 (so there are exact zeros, and negatives stay), and a row whose hidden pre-activation comes
    within the margin is drawn again.  -> dict: feats (R, ldf) with NaN in the padding columns, w1 (128, 1000), b1, w2 (nc, 128),
    dl (R, nc), ref = head_bwd_reference."""
    g = torch.Generator().manual_seed(R * 37 + nc)
    w1, b1 = torch.randn(HB_HID, HB_FEAT, generator=g) * 0.05, torch.randn(HB_HID, generator=g) * 0.1
    w2, dl = torch.randn(nc, HB_HID, generator=g) * 0.2, torch.randn(R, nc, generator=g)
    f = torch.empty(R, HB_FEAT)
    for r in range(R):
        for _ in range(100):
            row = torch.randn(HB_FEAT, generator=g)
            row[row.abs() < 0.05] = 0.0
            pre = torch.relu(row.double()) @ w1.double().T + b1.double()
            if float(pre.abs().min()) >= RELU_MARGIN:
                break
        f[r] = row
    feats = torch.full((R, ldf), float("nan"))
    feats[:, :HB_FEAT] = f
    c = {"feats": feats, "w1": w1, "b1": b1, "w2": w2, "dl": dl, "R": R, "nc": nc, "ldf": ldf, "ldd": ldd}
    c["ref"] = head_bwd_reference(f, w1, b1, w2, dl)
    assert c["ref"]["margin"] >= RELU_MARGIN and bool((f == 0).any()) and bool((f < 0).any()) and float(c["ref"]["d_h"].max()) < RELU_MARGIN
    return c


def head_bwd_reference(f, w1, b1, w2, dl):
    """fp64 backward of ReLU-Linear-ReLU-Linear and the bounds of the module docstring -> dict of (name, b_name) pairs; margin: the
    smallest distance of a ReLU argument from zero (exact zeros of the features apart)."""
    f, w1, b1, w2, dl = (t.double() for t in (f, w1, b1, w2, dl))
    R, nc = dl.shape
    rf = torch.relu(f)
    pre = rf @ w1.T + b1
    d_h = 503 * EPS * (rf @ w1.abs().T + b1.abs())
    h, on = torch.relu(pre), (pre > 0).double()
    dh = (dl @ w2) * on
    d_dh = (nc + 1) * EPS * (dl.abs() @ w2.abs()) * on
    fon = (f > 0).double()
    df = (dh @ w1) * fon
    nz = f[f != 0].abs()
    return {"margin": min(float(pre.abs().min()), float(nz.min()) if nz.numel() else float("inf")), "d_h": d_h,
            "dw1": dh.T @ rf, "b_dw1": d_dh.T @ rf + (R + 1) * EPS * (dh.abs().T @ rf),
            "db1": dh.sum(0), "b_db1": d_dh.sum(0) + R * EPS * dh.abs().sum(0),
            "dw2": dl.T @ h, "b_dw2": dl.abs().T @ d_h + (R + 1) * EPS * (dl.abs().T @ h),
            "db2": dl.sum(0), "b_db2": R * EPS * dl.abs().sum(0),
            "dfeats": df, "b_dfeats": U * df.abs() + ((d_dh @ w1.abs()) + 129 * EPS * (dh.abs() @ w1.abs())) * fon}


def emu_head_bwd(c):
    """f32 evaluation of the head's backward (torch's own summation order: the bounds hold for any order) -> dict like the reference"""
    f = c["feats"][:, :HB_FEAT]
    rf = torch.relu(f)
    h = torch.relu(rf @ c["w1"].T + c["b1"])
    dh = (c["dl"] @ c["w2"]) * (h > 0)
    return {"dw1": dh.T @ rf, "db1": dh.sum(0), "dw2": c["dl"].T @ h, "db2": c["dl"].sum(0), "dfeats": bf((dh @ c["w1"]) * (f > 0))}


# ------------------------------------------------------------------------------------------------ loss
LOSS_SHAPES = [(1, 2), (5, 5), (256, 5), (257, 5), (600, 32), (3, 1)]             # B, nc
LOSS_WEIGHTS = [(1.0 / 6.0, 5.0 / 6.0), (1.0, 0.0), (0.0, 1.0)]
LOSS_MUTANTS = ("smoothing_0.11", "focal_mean_over_b", "drop_om")


def _onehot(labels, nc):
    return torch.nn.functional.one_hot(labels.long(), nc).double()


def loss_reference(logits, labels, w_ls, w_fo):
    """oracle.train in float64 with autograd (w_ls lsce + w_fo focal, which is build_loss at the default weights: asserted) and
    the bounds of the module docstring -> dict: loss, grad, b_loss, b_grad."""
    assert float(logits.abs().max()) <= LOGIT_RANGE                       # the reference's own domain
    B, nc = logits.shape
    x = logits.double().clone().requires_grad_(True)
    t = _onehot(labels, nc)
    loss = w_ls * ot.lsce(x, t) + w_fo * ot.focal(x, t)
    if (w_ls, w_fo) == LOSS_WEIGHTS[0]:
        assert abs(float(loss.detach()) - float(ot.build_loss(x.detach(), t))) <= 1e-14 * abs(float(loss.detach()))
    loss.backward()
    grad, x = x.grad, x.detach()
    z = x - x.max(1, keepdim=True).values
    e = torch.exp(z)
    p = e / e.sum(1, keepdim=True)
    rel_e = EPS * z.abs() + 2 * EPS
    d_p = p * (rel_e + rel_e.max(1, keepdim=True).values + nc * EPS + EPS)
    c09 = 0.9 * t + 0.1 / nc
    g_ls = (p - c09) / B
    d_gls = (d_p + 3 * EPS * (p + c09) + 2 * EPS * (p - c09).abs()) / B
    bce = torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
    d_bce = 8 * EPS * bce
    pt = torch.exp(-bce)
    d_pt = pt * (d_bce + 2 * EPS)
    om = 1 - pt
    d_om = d_pt + EPS * om
    sig = torch.sigmoid(x)
    s = sig - t
    d_s = 5 * EPS * sig + EPS * s.abs()
    inner = 2 * pt * bce + om
    d_inner = 2 * ((pt + d_pt) * (bce + d_bce) - pt * bce) + 2 * EPS * pt * bce + d_om + 2 * EPS * inner
    g_fo = s * om * inner / (B * nc)
    d_gfo = ((s.abs() + d_s) * (om + d_om) * (inner + d_inner) - s.abs() * om * inner) / (B * nc) + 5 * EPS * g_fo.abs()
    b_grad = w_ls * d_gls + w_fo * d_gfo + 2 * EPS * ((w_ls * g_ls).abs() + (w_fo * g_fo).abs()) + EPS * grad.abs()
    nl = -torch.log(p)
    d_nl = d_p / p + 2 * EPS * nl.abs()
    row_ls = (0.9 * (nl * t).sum(1) + 0.1 * nl.sum(1) / nc) / B
    d_row_ls = (0.9 * (d_nl * t).sum(1) + 0.1 * (d_nl.sum(1) + nc * EPS * nl.sum(1)) / nc) / B + 6 * EPS * row_ls
    fl = om * om * bce
    d_fl = (om + d_om) ** 2 * (bce + d_bce) - fl + 3 * EPS * fl
    row_fo = fl.sum(1) / (B * nc)
    d_row_fo = (d_fl.sum(1) + nc * EPS * fl.sum(1)) / (B * nc) + 3 * EPS * row_fo
    v = w_ls * row_ls + w_fo * row_fo
    d_v = w_ls * d_row_ls + w_fo * d_row_fo + 3 * EPS * v
    b_loss = d_v.sum() + ((B + 255) // 256 + 9) * EPS * v.sum()
    return {"loss": loss.detach(), "grad": grad, "b_loss": b_loss, "b_grad": b_grad}


@functools.lru_cache(maxsize=None)
def loss_case(B, nc, w_ls, w_fo):
    """logits uniform in +-LOGIT_RANGE, with the extremes and an exact 0 planted; labels cover class 0 and nc - 1."""
    g = torch.Generator().manual_seed(B * 41 + nc)
    logits = (torch.rand(B, nc, generator=g) * 2 - 1) * LOGIT_RANGE
    flat = logits.view(-1)
    flat[0] = LOGIT_RANGE
    flat[-1] = -LOGIT_RANGE
    if flat.numel() > 2:
        flat[1] = 0.0
    labels = torch.randint(0, nc, (B,), generator=g, dtype=torch.int32)
    labels[0], labels[-1] = 0, nc - 1
    return {"logits": logits, "labels": labels, "ref": loss_reference(logits, labels, w_ls, w_fo)}


def emu_loss(logits, labels, w_ls, w_fo, mutant=None):
    """f32 emulation of loss_kernel, class by class in its order -> (loss, grad)."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    B, nc = logits.shape
    x, t = logits.float(), _onehot(labels, nc).float()
    inv_b, inv_c = f(1.0) / f(float(B)), f(1.0) / f(float(nc))
    inv_bc = inv_b if mutant == "focal_mean_over_b" else f(1.0) / (f(float(B)) * f(float(nc)))
    keep, sm = (f(0.89), f(0.11)) if mutant == "smoothing_0.11" else (f(0.9), f(0.1))
    w_ls, w_fo = f(w_ls), f(w_fo)
    e = torch.exp(x - x.max(1, keepdim=True).values)
    den = torch.zeros(B)
    for c in range(nc):
        den = den + e[:, c]
    cross, smooth, fl, grad = torch.zeros(B), torch.zeros(B), torch.zeros(B), torch.empty(B, nc)
    for c in range(nc):
        p, xc, tc = e[:, c] / den, x[:, c], t[:, c]
        nl = -torch.log(p)
        smooth = smooth + nl
        cross = cross + nl * tc
        bce = torch.clamp(xc, min=0) - xc * tc + torch.log1p(torch.exp(-xc.abs()))
        pt = torch.exp(-bce)
        om = f(1.0) - pt
        fl = fl + om * om * bce
        sig = f(1.0) / (f(1.0) + torch.exp(-xc))
        g_ls = (p - keep * tc - sm * inv_c) * inv_b
        g_fo = (sig - tc) * (f(1.0) if mutant == "drop_om" else om) * (f(2.0) * pt * bce + om) * inv_bc
        grad[:, c] = g_ls * w_ls + g_fo * w_fo
    v = (keep * cross + sm * smooth * inv_c) * inv_b * w_ls + fl * inv_bc * w_fo
    trips = (B + 255) // 256
    vt = torch.cat([v, torch.zeros(trips * 256 - B)]).reshape(trips, 256)
    acc = vt[0].clone()
    for k in range(1, trips):
        acc = acc + vt[k]
    w = acc.reshape(4, 64)
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, idx ^ o]
    return ((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0], grad


# ------------------------------------------------------------------------------------------------ SGD
SGD_NS = (1, 2, 3, 4, 5, 2048 * 256 * 4 + 7)          # the last: a second grid-stride trip of sgd_kernel (2048 workgroups) and a tail


def sgd_reference(p, g, m, lr, grad_scale, first, momentum=0.9, weight_decay=1e-3):
    """oracle.train.sgd_step in f32, one rounding per operation (the kernel's __f*_rn sequence); m is not read when first.
    -> (p_new, m_new, bf16 mirror of p_new)"""
    pn, mn = ot.sgd_step(p, g * grad_scale, None if first else m, lr, momentum, weight_decay)
    return pn, mn, bf(pn)
