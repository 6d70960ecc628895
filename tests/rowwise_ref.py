"""Plain fp64 restatements of the row-wise kernels between the Qwen3 GEMMs, and the checkers that compare a result with them.

Every function here is written from the formula, in torch fp64, on whatever device its operands live on; nothing is shared with the
kernels. Each operation is checked in two forms (the convention of tests/test_qwen_loss_head_gpu.py):

  * tight - against fp64 with the kernel's documented rounding points applied. A value that is rounded once from an f32 quantity v is
    accepted when |got - v| <= ulp/2 + e: half a bf16 ulp of the value (the rounding itself - never more than one ulp away from the
    rounded reference) plus e, the f32 error of v, written out next to its constant. A value behind TWO roundings (bf16(w * bf16(x *
    rstd)), bf16(bf16(silu(g)) * u), the RoPE sums) is exact once the inner bf16 value is known, because a product of two bf16 values
    is exact in f32: the inner value can only be the fp64 one or - when x * rstd sits within the f32 error of a rounding boundary - its
    neighbour, so the result must EQUAL one of the candidates built from rstd (1 -+ delta). Such checks report ratio 0 or >= 2.
  * loose - against the unrounded fp64 function, with the bound propagated to first order from the rounding points, per element,
    scaled by the sum of the absolute values of the terms (RoPE and g - xhat * dot cancel), never by the result.

Symbols: U = 2^-8 (bf16 unit roundoff), E = 2^-24 (f32 unit roundoff). A sum of n f32 terms in any order is off by at most
(n - 1) E sum|terms| to first order; `depth` below is the longest chain of additions one term passes through. TINY = 2^-126: f32 / bf16
smallest normal - v_rcp_f32 and v_rsq_f32 flush denormal results, so every absolute error carries a TINY-sized floor."""
import math

import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -8
E = 2.0 ** -24
TINY = 2.0 ** -126
BF16_MAX = 3.3895313892515355e38
RATIOS = {}            # name -> largest err / bound seen (the host test prints its table from here)


def bf(x):
    """Round to bf16 and back to fp64 (the kernels' rounding point)."""
    return x.to(BF16).to(F64)


def ulp(v):
    """The bf16 spacing at |v| (fp64 tensor): 2^(e - 8) for |v| = m 2^e, m in [0.5, 1); 2^-133 below the smallest normal."""
    _, e = torch.frexp(v.abs().clamp_min(TINY))
    return torch.ldexp(torch.ones_like(v), e - 8)


def report(name, err, bound):
    """Assert err <= bound elementwise and print / record the largest ratio."""
    err, bound = torch.as_tensor(err, dtype=F64), torch.as_tensor(bound, dtype=F64)
    bound = bound.expand_as(err)
    ratio = (err / bound).max().item() if err.numel() else 0.0
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio) if ratio == ratio else float("nan")
    print(f"\nTOL {name}: max err/bound {ratio:.3f} (max err {err.max().item() if err.numel() else 0:.3e})", end="")
    bad = (~(err <= bound)).nonzero()
    assert bad.shape[0] == 0, f"{name}: {bad.shape[0]} elements over bound, first {bad[:4].tolist()}: err " \
                              f"{err[tuple(bad[:4].T)].tolist()} bound {bound[tuple(bad[:4].T)].tolist()}"
    return ratio


def once(name, got, v, e):
    """Tight check of a value rounded once to bf16 from an f32 quantity: |got - v| <= ulp(|v| + e) / 2 + e."""
    got = got.to(F64)
    return report(name, (got - v).abs(), ulp(v.abs() + e) / 2 + e)


def among(name, got, cands):
    """Tight check of a value that is exact given its inner rounded operand: got must equal one of the candidates. Reported in units of
    half an ulp, so a match is 0 and the nearest possible miss is 2."""
    got = got.to(F64)
    d = torch.stack([(got - c).abs() for c in cands]).amin(0)
    return report(name, d, ulp(cands[0]) / 2)


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16 if a.element_size() == 2 else torch.int32),
                                                                     b.contiguous().view(torch.int16 if b.element_size() == 2 else torch.int32))


def rstd_rel(per_lane, levels):
    """Relative f32 error of rstd = rsqrtf(sum(x^2) / n + eps): a lane adds per_lane squares (each product E, each add E - all terms
    positive, so the error is relative to the sum: (per_lane + 1) E), the butterfly adds `levels` more; the power -1/2 halves it; the
    division and the + eps round once each (halved: E in all); v_rsq_f32 is good to one ulp = 2 E."""
    return ((per_lane + 1 + levels) / 2 + 1 + 2) * E


def colsum_depth(nrows):
    """Longest chain of f32 additions in the column-sum kernels: a row group walks nrows / 16 rows on 4 accumulators (nrows / 64, the tail
    adds up to 3 to the first), 2 levels join them, 15 adds join the 16 row groups, 1 for accumulate. The split form (512-row chunks,
    then nsplit <= nrows / 512 adds) is never longer than this."""
    return nrows / 64.0 + 4 + 2 + 15 + 1


# ================================================================================================ RMSNorm
def rms_stats(x, eps):
    x = x.to(F64)
    return torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)


def check_rmsnorm_fwd(tag, y, rstd, x, w, eps):
    """y = bf16(w * bf16(x * rstd)), rstd = (mean(x^2) + eps)^-1/2 over the row; x, w bf16, y bf16 [rows, cols], rstd f32 [rows] or None."""
    cols = x.shape[-1]
    x64, w64 = x.to(F64), w.to(F64)
    rs = rms_stats(x, eps)
    d = rstd_rel(8 * math.ceil(cols / 512), 6)             # a lane holds 8 values of every 512-column chunk; 64-lane butterfly: 6 levels
    if rstd is not None:
        report(tag + " rstd", (rstd.to(F64)[:, None] - rs).abs(), d * rs)
    # tight: x * rstd rounds in f32 first (E) and carries rstd's error d: the inner value is bf16(x rstd (1 -+ (d + E)))
    cands = [bf(w64 * bf(x64 * rs * (1 + s * (d + E)))) for s in (0, -1, 1)]
    among(tag + " y tight", y, cands)
    # loose: two roundings in sequence, (1 + U)^2 - 1 = 2U + U^2, plus rstd's error
    yl = w64 * x64 * rs
    report(tag + " y loose", (y.to(F64) - yl).abs(), (2 * U + U * U + d + E) * yl.abs() + TINY)


def rms_bwd64(dy, x, w, rs, dres=None):
    """fp64 RMSNorm backward from the saved rstd: dx = rstd (g - xh mean(g xh)) [+ dres], g = dy w, xh = x rstd; dw = sum_rows dy xh.
    Also returns the sums of absolute values the error bounds scale by."""
    dy, x, w, rs = dy.to(F64), x.to(F64), w.to(F64), rs.to(F64).reshape(-1, 1)
    xh, g = x * rs, dy * w
    dot = (g * xh).mean(-1, keepdim=True)
    adot = (g * xh).abs().mean(-1, keepdim=True)
    dx = rs * (g - xh * dot)
    adx = rs * (g.abs() + xh.abs() * adot)
    if dres is not None:
        dx = dx + dres.to(F64)
        adx = adx + dres.to(F64).abs()
    return dx, dy * xh, adx, adot


def check_rmsnorm_bwd_dx(tag, dx, dy, x, w, rstd, dres=None):
    """f32 error of dx before its one rounding, relative to A = rstd (|g| + |xh| mean|g xh|) + |dres|: xh rounds once (E), g = dy w is
    exact (bf16 x bf16), g xh rounds (E); the dot product adds 8 ceil(cols / 512) terms per lane and 6 butterfly levels and is divided
    by cols (E): its error is (depth + 3) E mean|g xh|; xh * dot (2 E), the subtraction, the product with rstd and the + dres round
    once each: 5 E A in all, plus the dot's."""
    cols = x.shape[-1]
    ref, _, adx, adot = rms_bwd64(dy, x, w, rstd, dres)
    depth = 8 * math.ceil(cols / 512) + 6
    rs, xh = rstd.to(F64).reshape(-1, 1), x.to(F64) * rstd.to(F64).reshape(-1, 1)
    e = 5 * E * adx + (depth + 3) * E * rs * xh.abs() * adot + TINY
    once(tag + " dx tight", dx, ref, e)
    report(tag + " dx loose", (dx.to(F64) - ref).abs(), U * ref.abs() + e)          # the one output rounding, first order


def check_colsum(tag, got, terms, depth, e_terms=0.0, old=None, out_bf16=True):
    """got[c] = [old[c] +] sum_r terms[r, c], accumulated in f32 along chains of at most `depth` additions, rounded once to bf16 (or
    left in f32): |f32 sum - sum| <= depth E sum|terms| + sum(e_terms), e_terms the error each term arrives with; old + new adds in f32
    (E) before the single rounding, so accumulate=True costs no second bf16 rounding in the tight form. Per column, never a norm."""
    t = terms.to(F64)
    ref = t.sum(0)
    e = depth * E * t.abs().sum(0) + (e_terms.sum(0) if torch.is_tensor(e_terms) else e_terms) + TINY
    if old is not None:
        ref = ref + old.to(F64)
        e = e + E * ref.abs() + E * old.to(F64).abs()
    if out_bf16:
        once(tag + " tight", got, ref, e)
        report(tag + " loose", (got.to(F64) - ref).abs(), U * ref.abs() + e)
    else:
        report(tag, (got.to(F64) - ref).abs(), E * ref.abs() + e)


def check_rmsnorm_bwd_dw(tag, dw, dy, x, rstd, rows_per_part, old=None):
    """dw[c] = sum_rows dy xh: a term rounds twice (xh, the product: 2 E each term); a wave adds rows_per_part / 4 rows in registers, 3
    adds join the 4 waves, then the column sum of ceil(rows / rows_per_part) partial rows."""
    rows = x.shape[0]
    terms = dy.to(F64) * x.to(F64) * rstd.to(F64).reshape(-1, 1)
    depth = rows_per_part / 4 + 3 + colsum_depth(math.ceil(rows / rows_per_part))
    check_colsum(tag + " dw", dw, terms, depth + 2, old=old)


# ================================================================================================ LayerNorm
def ln_parts(x, res, eps, x_bf16):
    """s = x + res (rounded to bf16 when the operands are bf16 tensors), mean, centred d, rstd - fp64. With the f32 errors:
    mean: a lane adds cols / 64 values, 6 butterfly levels, one division: em = (cols / 64 + 7) E mean|s| (+ E |s| for an f32 x + res);
    var: d carries em + E |d|, d^2 and the sum (cols / 64 + 8) E relative: ev = 2 mean|d| em + (cols / 64 + 10) E var;
    rstd: relative ev / (2 (var + eps)) + 3 E (the + eps, v_rsq_f32's ulp)."""
    cols = x.shape[-1]
    s = x.to(F64)
    es = torch.zeros_like(s)
    if res is not None:
        s = s + res.to(F64)
        if x_bf16:
            s = bf(s)
        else:
            es = E * s.abs()
    mean = s.mean(-1, keepdim=True)
    d = s - mean
    var = d.pow(2).mean(-1, keepdim=True)
    rs = torch.rsqrt(var + eps)
    em = (cols / 64 + 7) * E * s.abs().mean(-1, keepdim=True) + es.mean(-1, keepdim=True)
    ev = 2 * d.abs().mean(-1, keepdim=True) * em + (cols / 64 + 10) * E * var
    rrel = ev / (2 * (var + eps)) + 3 * E
    ed = em + es + E * d.abs()                                  # error of the centred value
    return s, mean, d, rs, ed, rrel


def check_layernorm_fwd(tag, yb, yf, x, res, w, b, eps):
    """y = (s - mean) rstd w + b, s = x (+ res); f32 statistics (two-pass variance); y f32 and / or bf16."""
    x_bf16 = x.dtype == BF16
    s, mean, d, rs, ed, rrel = ln_parts(x, res, eps, x_bf16)
    w64, b64 = w.to(F64), b.to(F64)
    ref = d * rs * w64 + b64
    # the centred value's error through rstd w; the products with rstd and w and the + b round once each: (rrel + 3 E) |d rstd w| + E |y|
    e = ed * (rs * w64).abs() + (rrel + 3 * E) * (d * rs * w64).abs() + E * ref.abs() + TINY
    if yf is not None:
        report(tag + " y_f32", (yf.to(F64) - ref).abs(), e)
    if yb is not None:
        once(tag + " y_bf16 tight", yb, ref, e)
    if x_bf16 and res is not None:
        # loose: the unrounded x + res. ds_j with |ds_j| <= U |s_j| reaches y_j as rstd w_j (ds_j - mean(ds) - xhat_j mean(xhat ds))
        sl = x.to(F64) + res.to(F64)
        ml = sl.mean(-1, keepdim=True)
        dl = sl - ml
        rl = torch.rsqrt(dl.pow(2).mean(-1, keepdim=True) + eps)
        xh = dl * rl
        refl = xh * w64 + b64
        prop = (rl * w64).abs() * U * (sl.abs() + sl.abs().mean(-1, keepdim=True) + xh.abs() * (xh * sl).abs().mean(-1, keepdim=True))
        for nm, got, out in (("y_f32", yf, E * refl.abs()), ("y_bf16", yb, U * refl.abs())):
            if got is not None:
                report(tag + f" {nm} loose", (got.to(F64) - refl).abs(), prop + e + out)


def check_layernorm_bwd(tag, dx, dw, db, dy, x, res, w, eps, dw_old=None, db_old=None):
    """dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy w; dw = sum_rows dy xhat; db = sum_rows dy - all f32, statistics recomputed."""
    rows, cols = x.shape
    s, mean, d, rs, ed, rrel = ln_parts(x, res, eps, False)
    dy64, w64 = dy.to(F64), w.to(F64)
    xh, g = d * rs, dy64 * w64
    mg, mgx = g.mean(-1, keepdim=True), (g * xh).mean(-1, keepdim=True)
    amg, amgx = g.abs().mean(-1, keepdim=True), (g * xh).abs().mean(-1, keepdim=True)
    ref = rs * (g - mg - xh * mgx)
    exh = ed * rs + (rrel + E) * xh.abs()                                 # xhat = d * rstd
    n = cols / 64 + 7                                                    # a row mean: cols / 64 adds per lane, 6 levels, the division
    emg = (n + 1) * E * amg                                              # g rounds once
    emgx = (n + 2) * E * amgx + (g.abs() * exh).mean(-1, keepdim=True)   # g, the fma, then xhat's own error
    # inside the bracket: g (E), the two subtractions and xhat * mgx (3 E of the absolute terms); then the product with rstd (rrel + E)
    brk = g.abs() + mg.abs() + (xh * mgx).abs()
    e = rs * (E * g.abs() + emg + exh * mgx.abs() + xh.abs() * emgx + 3 * E * brk) + (rrel + E) * rs * brk + TINY
    report(tag + " dx", (dx.to(F64) - ref).abs(), e)
    depth = 4 + 3 + colsum_depth(math.ceil(rows / 16))                   # 4 rows per wave, 3 adds across the waves, the column sum
    check_colsum(tag + " dw", dw, dy64 * xh, depth + 1, e_terms=dy64.abs() * exh, old=dw_old, out_bf16=False)
    check_colsum(tag + " db", db, dy64, depth, old=db_old, out_bf16=False)


# ================================================================================================ QK-RMSNorm + RoPE
def rot_half(t):
    h = t.shape[-1] // 2
    return torch.cat([-t[..., h:], t[..., :h]], -1)


def rope_tables(L, D=128, theta=5e6, device="cpu"):
    """cos / sin as Qwen3Model.rope builds them: fp32 angles, cat(freqs, freqs), cast to bf16."""
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.float) / D))
    fr = (inv[:, None] @ torch.arange(L, dtype=torch.float)[None, :]).transpose(0, 1)
    emb = torch.cat((fr, fr), dim=-1)
    return emb.cos().to(BF16).to(device).contiguous(), emb.sin().to(BF16).to(device).contiguous()


QK_RSTD_REL = rstd_rel(4, 5)      # a half-wave owns a 128-vector: 4 squares per lane, 5 butterfly levels: 7.5 E = 3.75 * 2^-23


def split_qkv(qkv, B, L, Hq, Hkv, D):
    t = qkv.reshape(B, L, Hq + 2 * Hkv, D)
    return t[:, :, :Hq], t[:, :, Hq:Hq + Hkv], t[:, :, Hq + Hkv:]


def check_qkprep_fwd(tag, Q, K, V, qr, kr, qkv, q_w, k_w, cos, sin, B, L, Hq, Hkv, eps, D=128):
    """Q, K [B, H, L, D] = rope(bf16(w * bf16(x * rstd))) per head vector, each RoPE product and their sum rounded to bf16; V a copy."""
    xq, xk, xv = split_qkv(qkv, B, L, Hq, Hkv, D)
    assert bits_equal(V, xv.transpose(1, 2).contiguous()), tag + ": V must be bit-equal to its input slice"
    c, s = cos.to(F64)[None, :, None, :], sin.to(F64)[None, :, None, :]
    for nm, got, x, w, r in (("Q", Q, xq, q_w, qr), ("K", K, xk, k_w, kr)):
        x64, w64 = x.to(F64), w.to(F64)
        rs = rms_stats(x, eps)                                          # [B, L, H, 1]
        if r is not None:
            report(f"{tag} {nm} rstd", (r.to(F64).reshape(B, L, -1, 1) - rs).abs(), QK_RSTD_REL * rs)
        got = got.to(F64).transpose(1, 2)                               # [B, L, H, D]
        # tight: the products n * cos are exact in f32 and the sum of two bf16 values rounds like fp64 does, so given the inner bf16
        # value everything is exact; the inner value of each of the two elements a result mixes is the fp64 one or its neighbour
        ns = [bf(w64 * bf(x64 * rs * (1 + sg * (QK_RSTD_REL + E)))) for sg in (-1, 1)]
        cands = [bf(bf(a * c) + bf(rot_half(b_) * s)) for a in ns for b_ in ns]
        among(f"{tag} {nm} tight", got, cands)
        # loose: n carries 2U + U^2, each product U, the sum U: (1 + U)^4 - 1 <= 4U + 7U^2 of |n cos| + |rot(n) sin|, plus rstd's error
        nl = w64 * x64 * rs
        ref = nl * c + rot_half(nl) * s
        mag = (nl * c).abs() + (rot_half(nl) * s).abs()
        report(f"{tag} {nm} loose", (got - ref).abs(), (4 * U + 7 * U * U + QK_RSTD_REL + 2 * E) * mag + TINY)


def qkprep_bwd64(dQ, dK, dV, qkv, q_w, k_w, cos, sin, qr, kr, B, L, Hq, Hkv, D=128):
    """fp64 backward from the saved row statistics; dK, dV [parts, B, Hkv, L, D] partial slabs, summed here. Returns per tensor the
    reference, the sum of absolute values it is built from, and the per-(token, head) terms of the norm-weight gradients."""
    xq, xk, _ = split_qkv(qkv, B, L, Hq, Hkv, D)
    c, s = cos.to(F64)[None, :, None, :], sin.to(F64)[None, :, None, :]
    out = {}
    for nm, dy, x, w, r in (("q", dQ.to(F64), xq, q_w, qr), ("k", dK.to(F64).sum(0), xk, k_w, kr)):
        ady = dQ.to(F64).abs() if nm == "q" else dK.to(F64).abs().sum(0)
        dy, ady = dy.transpose(1, 2), ady.transpose(1, 2)               # [B, L, H, D]
        # y = n cos + rot_half(n) sin  =>  dn = dy cos + rot_half^T(dy sin), rot_half^T(t) = cat(t2, -t1) = -rot_half(t)
        dn = dy * c - rot_half(dy * s)
        adn = ady * c.abs() + rot_half(ady * s.abs()).abs()
        rs = r.to(F64).reshape(B, L, -1, 1)
        xh = x.to(F64) * rs
        g, ag = dn * w.to(F64), adn * w.to(F64).abs()
        dot, adot = (g * xh).mean(-1, keepdim=True), (ag * xh.abs()).mean(-1, keepdim=True)
        out[nm] = (rs * (g - xh * dot), rs * (ag + xh.abs() * adot), dn * xh, adn * xh.abs())
    out["v"] = (dV.to(F64).sum(0).transpose(1, 2), dV.to(F64).abs().sum(0).transpose(1, 2))
    return out


def check_qkprep_bwd(tag, dqkv, dq_w, dk_w, dQ, dK, dV, qkv, q_w, k_w, cos, sin, qr, kr, B, L, Hq, Hkv, old_q=None, old_k=None, D=128):
    parts = dK.shape[0]
    ref = qkprep_bwd64(dQ, dK, dV, qkv, q_w, k_w, cos, sin, qr, kr, B, L, Hq, Hkv, D)
    gq, gk, gv = split_qkv(dqkv, B, L, Hq, Hkv, D)
    if parts == 1:
        assert bits_equal(gv.contiguous(), dV[0].transpose(1, 2).contiguous()), tag + ": dV with one slab must be bit-equal to its input"
    else:   # f32 sum of the slabs in slab order (parts - 1 adds), rounded once
        once(tag + " dv tight", gv, ref["v"][0], (parts - 1) * E * ref["v"][1] + TINY)
    sl = (parts - 1) if parts > 1 else 0
    for nm, got, wout, old, H in (("q", gq, dq_w, old_q, Hq), ("k", gk, dk_w, old_k, Hkv)):
        dx, adx, terms, aterms = ref[nm]
        s_ = sl if nm == "k" else 0
        # f32 error of dqkv relative to A = rstd (|dn| |w| + |xh| mean(|dn| |w| |xh|)) built from |dy cos| + |dy sin|: the slab sum
        # (parts - 1), dn's two products and their sum (3 E; the products are exact for a single bf16 slab), g = dn w (E), xh (E), the dot
        # of 4 products per lane and 5 butterfly levels and its division (4 + 5 + 3) E, xh * dot, the subtraction, the product with rstd
        # (3 E): 20 E + slab sum covers every path a term takes
        e = (20 + s_) * E * adx + TINY
        once(f"{tag} d{nm} tight", got, dx, e)
        report(f"{tag} d{nm} loose", (got.to(F64) - dx).abs(), U * dx.abs() + e)
        # norm-weight gradient, per column: a half-wave adds its heads (ceil(H / 8) per token ... at most ceil(HT / 8)) over 8 tokens in
        # registers, 7 adds join the 8 half-wave slots, then the column sum of ceil(T / 8) partial rows; a term dn * xh carries (5 + sl) E
        HT = Hq + 2 * Hkv
        depth = 8 * math.ceil(HT / 8) + 7 + colsum_depth(math.ceil(B * L / 8))
        t2 = terms.reshape(-1, D)
        check_colsum(f"{tag} d{nm}_w", wout, t2, depth, e_terms=(5 + s_) * E * aterms.reshape(-1, D), old=old)


# ================================================================================================ SwiGLU
def silu_err(g):
    """Relative f32 error of sigmoid(g) = v_rcp_f32(1 + __expf(-g)) (and so of silu = g * sigmoid, one more E): __expf scales the argument
    by log2(e) in f32, an absolute argument error E |g| log2(e) that the exponential turns into a relative one of 1.45 |g| E, and
    v_exp_f32 is good to one ulp (2 E); in 1 + e^-g that share weighs e^-g / (1 + e^-g) = 1 - sigmoid; the add E, v_rcp_f32 one ulp 2 E."""
    sg = torch.sigmoid(g)
    return ((1.45 * g.abs() + 2) * (1 - sg) + 3) * E


def check_silu_mul_fwd(tag, act, gu):
    """act = bf16(bf16(silu(g)) * u), gu = [g | u] bf16 [rows, 2 inter]. Compared wherever the fp64 result is finite in bf16; the result
    must be finite there. v_rcp_f32 flushes a denormal sigmoid (g < -87.3) to zero: an absolute error of TINY on the sigmoid, |g| TINY
    on silu, |g u| TINY on the product - the floor below."""
    inter = gu.shape[1] // 2
    g, u = gu[:, :inter].to(F64), gu[:, inter:].to(F64)
    sg = torch.sigmoid(g)
    sl = g * sg
    d = silu_err(g) + E
    floor = g.abs() * TINY
    cands = [bf(bf(sl * (1 + s * d) + t * floor) * u) for s, t in ((0, 0), (-1, -1), (1, 1), (-1, 1), (1, -1))]
    ref = sl * u
    fin = bf(bf(sl) * u).abs() <= BF16_MAX
    got = act.to(F64)
    assert torch.isfinite(got[fin]).all(), tag + ": non-finite act where the fp64 result is finite in bf16"
    lo, hi = torch.stack(cands).amin(0), torch.stack(cands).amax(0)
    # between the candidates (monotone in the inner value): distance outside [lo, hi], zero for a faithful kernel
    out = (lo - got).clamp_min(0) + (got - hi).clamp_min(0)
    report(tag + " act tight", out[fin], (ulp(cands[0]) / 2)[fin])
    report(tag + " act loose", (got - ref).abs()[fin], ((2 * U + U * U + d) * ref.abs() + (floor * u.abs()) * (1 + 2 * U) + TINY)[fin])


def check_silu_mul_bwd(tag, dgu, dact, gu):
    """d_gate = bf16(d u sigma (1 + g (1 - sigma))), d_up = bf16(d silu(g)): f32 throughout, one rounding each."""
    inter = gu.shape[1] // 2
    g, u, d = gu[:, :inter].to(F64), gu[:, inter:].to(F64), dact.to(F64)
    sg = torch.sigmoid(g)
    rel = silu_err(g)
    # d_up: silu's error, one product: (rel + 2 E) |d g sigma|, floor |d g| TINY (flushed sigmoid)
    ref_u = d * g * sg
    e_u = (rel + 2 * E) * ref_u.abs() + (d * g).abs() * TINY + TINY
    # d_gate = d u (sigma + g sigma (1 - sigma)): 1 - sigma carries rel sigma / (1 - sigma) - for g >> 0 it is 1 - (1 - tiny): absolute E;
    # the terms sigma and g sigma (1 - sigma) cancel for g < -1, so the bound scales by |sigma| + |g sigma (1 - sigma)|:
    # each carries 2 rel + 4 E, plus |g sigma| E for 1 - sigma's absolute error, then d u (2 E)
    t1, t2 = sg, g * sg * (1 - sg)
    ref_g = d * u * (t1 + t2)
    mag = (d * u).abs() * (t1.abs() + t2.abs())
    # the kernel multiplies the bounded factor t = sigma (1 + g (1 - sigma)) in first, d * (u * t): a flushed sigmoid makes t an exact zero
    # (absolute error (1 + |g|) TINY on t, |d u| times that on the result), and u * t may land among the f32 denormals, where its
    # rounding is absolute, half the denormal spacing 2^-150, carried to the result by |d|
    e_g = (2 * rel + 8 * E) * mag + (d * u * g * sg).abs() * 2 * E + (d * u).abs() * (1 + g.abs()) * 2 * TINY + d.abs() * 2.0 ** -150 + TINY
    got_g, got_u = dgu[:, :inter].to(F64), dgu[:, inter:].to(F64)
    for nm, got, ref, e in (("d_gate", got_g, ref_g, e_g), ("d_up", got_u, ref_u, e_u)):
        fin = torch.isfinite(bf(ref))                      # the fp64 result is finite in bf16: the kernel's must be finite too
        # (d = 3e38 with g = +3e38: d g is finite in fp64 but past BF16_MAX, so ref is infinite in bf16 and the element is masked out;
        # with g = -3e38 ref is 0 and e_u's floor |d g| TINY is vast, which leaves the finiteness assertion below as the check there)
        assert torch.isfinite(got[fin]).all(), f"{tag}: non-finite {nm} where the fp64 result is finite in bf16"
        once(f"{tag} {nm} tight", got[fin], ref[fin], e[fin])
        report(f"{tag} {nm} loose", (got - ref).abs()[fin], (U * ref.abs() + e)[fin])


# ================================================================================================ AdamW, sum of squares
def f32c(v):
    """A Python float as the C ABI passes it: rounded to f32."""
    return torch.tensor(v, dtype=F32).to(F64).item()


class AdamW64:
    """The fp64 recurrence with bias correction, decoupled weight decay, gscale and the global-norm clip coefficient
    min(1, max_norm / (sqrt(sumsq) gscale + 1e-6)), next to a running first-order bound on the f32 kernel's distance from it.
    Per step (operands as the kernel reads them: the scalars rounded to f32):
      coefficient: sqrt, product, + 1e-6, division, min, product with gscale: 6 E relative on g' = g * gscale'              -> rg = 7 E
      m' = b1 m + (1 - b1) g': (1 - b1) E, three products and a sum: em' = b1 em + 2 E |b1 m| + (rg + 4 E) |(1 - b1) g'|
      v' likewise with g'^2 (2 rg, one more product): ev' = b2 ev + 2 E |b2 v| + (2 rg + 6 E) |(1 - b2) g'^2|
      bc1 = 1 - powf(b1, t), bc2 = 1 - powf(b2, t) on the host in f32: powf is good to an ulp of b^t <= 1, so the difference is off by
        up to 2 E absolute - 2 E / bc relative (b2 = 0.999 at t = 1: 2000 E; the subtraction cancels). bc2s = sqrt(bc2) halves it (+ E).
      denom = sqrt(v') / bc2s + eps: |d sqrt(v')| <= min(ev' / (2 sqrt(v')), sqrt(ev')); (rel(bc2s) + 3 E) sqrt(v') / bc2s; E denom
      p' = p (1 - lr wd) - (lr / bc1) (m' / denom): ep' = ep + 3 E |p| + upd (rel(bc1) + 4 E) + (lr / bc1) (em' / denom + |m'| ed / denom^2)
    so a step adds a few E relative to the terms, and the bound accumulates over the steps."""

    def __init__(self, p, m, v, lr, b1, b2, eps, wd):
        self.p, self.m, self.v = p.to(F64).clone(), m.to(F64).clone(), v.to(F64).clone()
        self.lr, self.b1, self.b2, self.eps, self.wd = f32c(lr), f32c(b1), f32c(b2), f32c(eps), f32c(wd)
        self.ep, self.em, self.ev = (torch.zeros_like(self.p) for _ in range(3))

    def step(self, grad, step, gscale=1.0, sumsq=None, max_norm=0.0):
        g = grad.to(F64)
        gs = f32c(gscale)
        if sumsq is not None:
            total = math.sqrt(float(sumsq)) * gs
            gs = gs * min(1.0, f32c(max_norm) / (total + f32c(1e-6)))
        lr, b1, b2, eps, wd = self.lr, self.b1, self.b2, self.eps, self.wd
        g = g * gs
        rg = 7 * E
        self.em = b1 * self.em + 2 * E * (b1 * self.m).abs() + (rg + 4 * E) * ((1 - b1) * g).abs()
        self.ev = b2 * self.ev + 2 * E * (b2 * self.v).abs() + (2 * rg + 6 * E) * ((1 - b2) * g * g).abs()
        self.m = b1 * self.m + (1 - b1) * g
        self.v = b2 * self.v + (1 - b2) * g * g
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        r1, r2s = 2 * E / bc1 + E, E / bc2 + 2 * E
        sq = self.v.sqrt()
        esq = torch.minimum(self.ev / (2 * sq).clamp_min(1e-300), self.ev.sqrt())
        denom = sq / math.sqrt(bc2) + eps
        ed = esq / math.sqrt(bc2) + (r2s + 3 * E) * sq / math.sqrt(bc2) + E * denom
        upd = (lr / bc1) * self.m / denom
        self.ep = self.ep + 3 * E * self.p.abs() + upd.abs() * (r1 + 4 * E) + (lr / bc1) * (self.em / denom + self.m.abs() * ed / denom ** 2)
        self.p = self.p * (1 - lr * wd) - upd
        return self

    def check(self, tag, p, m, v, w):
        report(tag + " p", (p.to(F64) - self.p).abs(), self.ep + E * self.p.abs() + TINY)
        report(tag + " m", (m.to(F64) - self.m).abs(), self.em + E * self.m.abs() + TINY)
        report(tag + " v", (v.to(F64) - self.v).abs(), self.ev + E * self.v.abs() + TINY)
        assert bits_equal(w, p.to(BF16)), tag + ": w must be bf16(p) bit for bit"


def check_sumsq(tag, got, x, start):
    """got = start + sum(x^2) in f32: a thread adds n / (8 * 256 * blocks) vectors of 8 (4 for f32) squares, a 256-thread tree (8 levels),
    up to 1024 block partials on 256 threads (4) and a tree (8), then the + start: with at most 1024 blocks a thread sees at most
    n / 262144 + 1 vectors. All terms are positive, so the bound is relative to the result."""
    n = x.numel()
    ref = x.to(F64).pow(2).sum() + start
    depth = 8 * (n / 262144 + 1) + 8 + 4 + 8 + 1
    report(tag, (torch.as_tensor(got, dtype=F64) - ref).abs().reshape(1), ((depth + 1) * E * ref).reshape(1))
