"""The checkers of tests/rowwise_ref.py against a faithful implementation and against planted faults - no GPU needed.

(a) The same operations done the reference project's way - PyTorch on the CPU, bf16 tensors at Qwen3's rounding points, fp32 for the
LayerNorm ops, backward passes in fp32 rounded once to bf16 at the output - pass every tight and loose checker. Largest err / bound
of each check over the shapes below (printed by `pytest -s`; "exact" checks accept only the candidates an inner rounding allows, so
their ratio is 0 by construction and the 0.01 rule does not apply to them):

    check                          ratio      check                          ratio
    rmsnorm rstd                   0.11       qkprep Q / K rstd              0.26
    rmsnorm y tight (exact)        0.00       qkprep Q / K tight (exact)     0.00
    rmsnorm y loose                0.91       qkprep Q / K loose             0.84 / 0.67
    rmsnorm dx tight / loose       1.00 / 0.99  qkprep dq / dk tight         1.00 / 1.00
    rmsnorm dw tight / loose       1.00 / 0.98  qkprep dq / dk loose         0.99 / 0.99
    layernorm y_f32                0.16       qkprep dv tight                1.00
    layernorm y_bf16 tight         1.00       qkprep dq_w / dk_w tight       0.99 / 0.99
    layernorm y loose (bf16 + res) 0.55       qkprep dq_w / dk_w loose       0.96 / 0.95
    layernorm dx                   0.07       swiglu act tight (exact)       0.00
    layernorm dw / db              0.04 / 0.05  swiglu act loose             0.92
    column sum tight / loose       0.99 / 0.91  swiglu d_gate / d_up tight   1.00 / 1.00
    column sum f32                 0.06       swiglu d_gate / d_up loose     1.00 / 0.99
    sumsq                          0.03       adamw p / m / v                0.52 / 0.23 / 0.23
    (tight ratios near 1 are the half-ulp rounding itself, which the bound allows exactly)

(b) Each planted fault makes its checker raise."""
import math

import pytest
import torch

from tests import rowwise_ref as R
from tests.rowwise_ref import BF16, F32, F64

EPS = 1e-6


def rnd(shape, seed, scale=1.0, dtype=BF16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


# ------------------------------------------------------------------------------------------------ the faithful implementations
def rms_fwd(x, w, eps, fault=None):
    xf = x.float()
    rs = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    if fault == "rstd_neighbour":
        rs = torch.roll(rs, 1, 0)
    y = w * (xf * rs).to(BF16)
    if fault == "col_2ulp":
        y = y.clone()
        y[:, 5] = (y[:, 5].double() + 2 * R.ulp(y[:, 5].double())).to(BF16)
    return y, rs.squeeze(-1)


def rms_bwd(dy, x, w, rs, dres, rpp=4, fault=None):
    xh = x.float() * rs[:, None]
    g = dy.float() * w.float()
    dx = rs[:, None] * (g - xh * (g * xh).mean(-1, keepdim=True))
    if dres is not None:
        add = dres.float().clone()
        if fault == "dres_last_row":
            add[-1] = 0
        dx = dx + add
    t = dy.float() * xh
    rows = x.shape[0]
    nblk = (rows + rpp - 1) // rpp
    part = torch.zeros(nblk * rpp, x.shape[1])
    part[:rows] = t
    part = part.view(nblk, rpp, -1).sum(1)
    if fault == "dw_partial_dropped":
        part[-1] = 0
    return dx.to(BF16), part.sum(0).to(BF16)


def qk_fwd(qkv, qw, kw, cos, sin, B, L, Hq, Hkv, eps, fault=None):
    q, k, v = R.split_qkv(qkv, B, L, Hq, Hkv, 128)
    if fault == "table_row":
        cos, sin = torch.roll(cos, -1, 0), torch.roll(sin, -1, 0)
    c, s = cos[None, :, None, :], sin[None, :, None, :]
    outs, rs_ = [], []
    for t, w in ((q, qw), (k, kw)):
        rs = torch.rsqrt(t.float().pow(2).mean(-1, keepdim=True) + eps)
        n = w * (t.float() * rs).to(BF16)
        rh = R.rot_half(n) if fault != "rot_sign" else -R.rot_half(n)
        outs.append(((n * c) + (rh * s)).transpose(1, 2).contiguous())       # bf16 ops: each product and the sum round
        rs_.append(rs.reshape(-1))
    return outs[0], outs[1], v.transpose(1, 2).contiguous(), rs_[0], rs_[1]


def qk_bwd(dQ, dK, dV, qkv, qw, kw, cos, sin, qr, kr, B, L, Hq, Hkv, fault=None):
    q, k, _ = R.split_qkv(qkv, B, L, Hq, Hkv, 128)
    c, s = cos.float()[None, :, None, :], sin.float()[None, :, None, :]
    slabs = range(dK.shape[0]) if fault != "slab3" else range(3)
    dKs = sum(dK[i].float() for i in slabs)
    dVs = sum(dV[i].float() for i in slabs)
    res, dws = [], []
    for dy, x, w, r in ((dQ.float(), q, qw, qr), (dKs, k, kw, kr)):
        dy = dy.transpose(1, 2)
        dn = dy * c - R.rot_half(dy * s)
        rs = r.reshape(B, L, -1, 1)
        xh = x.float() * rs
        g = dn * w.float()
        res.append(rs * (g - xh * (g * xh).mean(-1, keepdim=True)))
        t = (dn * xh)
        if fault == "last_token" and len(dws) == 0:
            t = t.clone()
            t[-1, -1] = 0
        dws.append(t.reshape(-1, 128).sum(0).to(BF16))
    dv = (dV[0] if dV.shape[0] == 1 else dVs.to(BF16)).transpose(1, 2)
    dqkv = torch.cat([res[0].to(BF16), res[1].to(BF16), dv.to(BF16)], 2).reshape(B * L, -1)
    return dqkv, dws[0], dws[1]


def adamw(p, m, v, g, lr, b1, b2, eps, wd, step, gscale=1.0, sumsq=None, max_norm=0.0, fault=None):
    f = lambda a: torch.tensor(a, dtype=F32)
    gs = f(gscale)
    if sumsq is not None:
        gs = gs * torch.minimum(f(1.0), f(max_norm) / (torch.sqrt(f(sumsq)) * gs + f(1e-6)))
    gf = g.float() * gs
    m = f(b1) * m + (1 - f(b1)) * gf
    v = f(b2) * v + (1 - f(b2)) * gf * gf
    bc1 = 1 - f(b1) ** step
    bc2s = torch.sqrt(1 - f(b2) ** step) if fault != "no_bc2" else f(1.0)
    denom = v.sqrt() / bc2s + f(eps)
    if fault == "wd_new":
        p = p - (f(lr) / bc1) * (m / denom)
        p = p * (1 - f(lr) * f(wd))
    else:
        p = p * (1 - f(lr) * f(wd)) - (f(lr) / bc1) * (m / denom)
    return p, m, v, p.to(BF16)


# ------------------------------------------------------------------------------------------------ (a) + (b): RMSNorm
def rms_rows(rows, cols, seed):
    """Row kinds inside one tensor: N(0, 2), all-zero, 1e4, 1e-20 (squares underflow), one 3e4 spike among zeros."""
    x = rnd((rows, cols), seed, 2.0).float()
    if rows >= 5:
        x[1] = 0
        x[2] *= 1e4
        x[3] *= 1e-20
        x[4] = 0
        x[4, cols // 2] = 3e4
    return x.to(BF16)


@pytest.mark.parametrize("rows,cols", [(5, 8), (3, 520), (9, 1032), (21, 2560)])
def test_rmsnorm_faithful_passes(rows, cols):
    x, w = rms_rows(rows, cols, 1), (1 + rnd((cols,), 2, 0.2).float()).to(BF16)
    y, rs = rms_fwd(x, w, EPS)
    R.check_rmsnorm_fwd("host rmsnorm", y, rs, x, w, EPS)
    dy, dres = rnd((rows, cols), 3), rnd((rows, cols), 4)
    for dr in (None, dres):
        for rpp in (4, 16):
            dx, dw = rms_bwd(dy, x, w, rs, dr, rpp)
            R.check_rmsnorm_bwd_dx("host rmsnorm", dx, dy, x, w, rs, dr)
            R.check_rmsnorm_bwd_dw("host rmsnorm", dw, dy, x, rs, rpp)
    if rows >= 5:     # an all-zero row: rstd = eps^-1/2 and dx = rstd dy w
        assert abs(rs[1].item() - EPS ** -0.5) < 1e-3 * EPS ** -0.5
        dx, _ = rms_bwd(dy, x, w, rs, None)
        assert torch.isfinite(dx.float()).all() and torch.equal(dx[1], (rs[1] * dy[1].float() * w.float()).to(BF16))


@pytest.mark.parametrize("fault", ["col_2ulp", "rstd_neighbour"])
def test_rmsnorm_fwd_fault_is_caught(fault):
    x, w = rnd((9, 520), 1, 2.0) * (1 + torch.arange(9)[:, None]).to(BF16), (1 + rnd((520,), 2, 0.2).float()).to(BF16)
    y, rs = rms_fwd(x, w, EPS, fault)
    with pytest.raises(AssertionError, match={"col_2ulp": "fault y tight", "rstd_neighbour": "fault rstd"}[fault]):
        R.check_rmsnorm_fwd("fault", y, rs, x, w, EPS)


@pytest.mark.parametrize("fault", ["dres_last_row", "dw_partial_dropped"])
def test_rmsnorm_bwd_fault_is_caught(fault):
    rows, cols = 1201, 128
    x, w = rnd((rows, cols), 1, 2.0), (1 + rnd((cols,), 2, 0.2).float()).to(BF16)
    _, rs = rms_fwd(x, w, EPS)
    dy, dres = rnd((rows, cols), 3), rnd((rows, cols), 4)
    dx, dw = rms_bwd(dy, x, w, rs, dres, 4, fault)
    if fault == "dres_last_row":          # the other output is untouched by the fault and still passes
        R.check_rmsnorm_bwd_dw("fault", dw, dy, x, rs, 4)
        with pytest.raises(AssertionError, match="fault dx tight"):
            R.check_rmsnorm_bwd_dx("fault", dx, dy, x, w, rs, dres)
    else:
        R.check_rmsnorm_bwd_dx("fault", dx, dy, x, w, rs, dres)
        with pytest.raises(AssertionError, match="fault dw tight"):
            R.check_rmsnorm_bwd_dw("fault", dw, dy, x, rs, 4)


# ------------------------------------------------------------------------------------------------ column sums, sum of squares
@pytest.mark.parametrize("nrows,cols", [(1, 8), (17, 72), (130, 64), (1025, 128)])
def test_colsum_faithful_passes_and_skipped_row_is_caught(nrows, cols):
    part = rnd((nrows, cols), 5, 1.0, F32)
    old = rnd((cols,), 6)
    R.check_colsum("host colsum", part.sum(0).to(BF16), part, R.colsum_depth(nrows))
    R.check_colsum("host colsum acc", (part.sum(0) + old.float()).to(BF16), part, R.colsum_depth(nrows), old=old)
    R.check_colsum("host colsum f32", part.sum(0), part, R.colsum_depth(nrows), out_bf16=False)
    ints = torch.randint(-8, 9, (nrows, cols), generator=torch.Generator().manual_seed(7)).float()
    with pytest.raises(AssertionError, match="fault tight"):
        R.check_colsum("fault", (ints.sum(0) - ints[-1] + (ints[-1] == 0)).to(BF16), ints, R.colsum_depth(nrows))
    with pytest.raises(AssertionError, match="fault: "):
        R.check_colsum("fault", part[:-1].sum(0) + (part[-1] == 0), part, R.colsum_depth(nrows), out_bf16=False)


@pytest.mark.parametrize("dt,n", [(BF16, 1023), (F32, 1000003), (F32, 3)])
def test_sumsq_faithful_passes(dt, n):
    x = rnd((n,), 8, 1.0, dt)
    R.check_sumsq("host sumsq", (x.float().pow(2).sum() + 2.5).item(), x, 2.5)
    if n <= 1023:      # (at 1e6 elements one element is below the f32 sum's own error)
        with pytest.raises(AssertionError, match="fault: "):
            R.check_sumsq("fault", (x[:-1].float().pow(2).sum() + 2.5).item() - 1e-2, x, 2.5)


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("rows,cols", [(5, 4), (13, 252), (17, 1028), (19, 2048)])
def test_layernorm_faithful_passes(rows, cols):
    F = torch.nn.functional
    w, b = 1 + rnd((cols,), 9, 0.2, F32), rnd((cols,), 10, 0.2, F32)
    for dt in (F32, BF16):
        x = (rnd((rows, cols), 11, 1.0, F32) + torch.tensor([0.0, 1e3] * rows)[:rows, None]).to(dt)   # mean 1e3, std 1: cancellation
        for res in (None, rnd((rows, cols), 12, 1.0, dt)):
            s = x if res is None else x + res
            y = F.layer_norm(s.float(), (cols,), w, b, EPS)
            R.check_layernorm_fwd(f"host layernorm {dt}", y.to(BF16), y, x, res, w, b, EPS)
    x, res, dy = rnd((rows, cols), 13, 1.0, F32) + 3, rnd((rows, cols), 14, 1.0, F32), rnd((rows, cols), 15, 1.0, F32)
    for r in (None, res):
        xa = x.clone().requires_grad_(True)
        wa, ba = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        F.layer_norm(xa if r is None else xa + r, (cols,), wa, ba, EPS).backward(dy)
        R.check_layernorm_bwd("host layernorm", xa.grad, wa.grad, ba.grad, dy, x, r, w, EPS)
    with pytest.raises(AssertionError, match="fault db"):   # the last row's dy missing from db (dx and dw come first and pass)
        R.check_layernorm_bwd("fault", xa.grad, wa.grad, ba.grad - dy[-1] - (dy[-1] == 0).float(), dy, x, res, w, EPS)


# ------------------------------------------------------------------------------------------------ QK-norm + RoPE
def qk_case(B, L, Hq, Hkv, parts, seed):
    HT = Hq + 2 * Hkv
    qkv = rnd((B * L, HT * 128), seed, 1.5)
    qw, kw = (1 + rnd((128,), seed + 1, 0.3).float()).to(BF16), (1 + rnd((128,), seed + 2, 0.3).float()).to(BF16)
    cos, sin = R.rope_tables(L)
    dQ = rnd((B, Hq, L, 128), seed + 3)
    dK, dV = rnd((parts, B, Hkv, L, 128), seed + 4), rnd((parts, B, Hkv, L, 128), seed + 5)
    return qkv, qw, kw, cos, sin, dQ, dK, dV


@pytest.mark.parametrize("Hq,Hkv,B,L,parts", [(8, 2, 1, 7, 1), (1, 1, 3, 5, 2), (5, 3, 1, 33, 4), (40, 8, 1, 9, 3)])
def test_qkprep_faithful_passes(Hq, Hkv, B, L, parts):
    qkv, qw, kw, cos, sin, dQ, dK, dV = qk_case(B, L, Hq, Hkv, parts, 20)
    Q, K, V, qr, kr = qk_fwd(qkv, qw, kw, cos, sin, B, L, Hq, Hkv, EPS)
    R.check_qkprep_fwd("host qkprep", Q, K, V, qr, kr, qkv, qw, kw, cos, sin, B, L, Hq, Hkv, EPS)
    dqkv, dqw, dkw = qk_bwd(dQ, dK, dV, qkv, qw, kw, cos, sin, qr, kr, B, L, Hq, Hkv)
    R.check_qkprep_bwd("host qkprep", dqkv, dqw, dkw, dQ, dK, dV, qkv, qw, kw, cos, sin, qr, kr, B, L, Hq, Hkv)


@pytest.mark.parametrize("fault", ["rot_sign", "table_row"])
def test_qkprep_fwd_fault_is_caught(fault):
    B, L, Hq, Hkv = 1, 33, 5, 3
    qkv, qw, kw, cos, sin, *_ = qk_case(B, L, Hq, Hkv, 1, 21)
    Q, K, V, qr, kr = qk_fwd(qkv, qw, kw, cos, sin, B, L, Hq, Hkv, EPS, fault)
    with pytest.raises(AssertionError, match="fault Q tight"):      # V and the rstd side outputs come first and pass
        R.check_qkprep_fwd("fault", Q, K, V, qr, kr, qkv, qw, kw, cos, sin, B, L, Hq, Hkv, EPS)


@pytest.mark.parametrize("fault", ["last_token", "slab3"])
def test_qkprep_bwd_fault_is_caught(fault):
    B, L, Hq, Hkv = 1, 33, 5, 3
    qkv, qw, kw, cos, sin, dQ, dK, dV = qk_case(B, L, Hq, Hkv, 4, 22)
    _, _, _, qr, kr = qk_fwd(qkv, qw, kw, cos, sin, B, L, Hq, Hkv, EPS)
    out = qk_bwd(dQ, dK, dV, qkv, qw, kw, cos, sin, qr, kr, B, L, Hq, Hkv, fault)
    # last_token: dv, dq come first and pass, dq_w trips; slab3: the summed dV misses its fourth slab
    with pytest.raises(AssertionError, match={"last_token": "fault dq_w tight", "slab3": "fault dv tight"}[fault]):
        R.check_qkprep_bwd("fault", *out, dQ, dK, dV, qkv, qw, kw, cos, sin, qr, kr, B, L, Hq, Hkv)


# ------------------------------------------------------------------------------------------------ SwiGLU
def swiglu_case(rows, inter, seed):
    """N(0, 1.5) with the edge gates against every edge up / dact value in the first rows."""
    gu, dact = rnd((rows, 2 * inter), seed, 1.5).float(), rnd((rows, inter), seed + 1).float()
    gates = [0.0, -0.0, 1e-30, -1e-30, 20, -20, 87, -87, 89, -89, 200, -200, 3e38, -3e38, R.BF16_MAX, -R.BF16_MAX]
    edge = [0.0, 3e38, -3e38, 1.0]
    k = 0
    for gte in gates:
        for uu in edge:
            for dd in edge:
                r, c = divmod(k, inter)
                if r < rows:
                    gu[r, c], gu[r, inter + c], dact[r, c] = gte, uu, dd
                k += 1
    return gu.to(BF16), dact.to(BF16)


@pytest.mark.parametrize("rows,inter", [(1, 8), (3, 136), (40, 256)])
def test_swiglu_faithful_passes(rows, inter):
    gu, dact = swiglu_case(rows, inter, 30)
    g, u = gu[:, :inter], gu[:, inter:]
    act = torch.nn.functional.silu(g) * u
    R.check_silu_mul_fwd("host swiglu", act, gu)
    # backward: fp32 math rounded once. The bounded factor is multiplied in first, as the kernel does: d * u formed first is inf at the
    # edge values (3e38 * 3e38) and inf * sigmoid(-3e38) = inf * 0 = NaN where the true gradient is 0
    gf, uf, df = g.float(), u.float(), dact.float()
    sg = torch.sigmoid(gf)
    dgu = torch.cat([(df * (uf * (sg * (1 + gf * (1 - sg))))).to(BF16), (df * (gf * sg)).to(BF16)], 1)
    R.check_silu_mul_bwd("host swiglu", dgu, dact, gu)
    bad = act.clone()
    bad[0, 7] = (bad[0, 7].double() + 2 * R.ulp(bad[0, 7].double())).to(BF16)
    with pytest.raises(AssertionError, match="fault act tight"):
        R.check_silu_mul_fwd("fault", bad, gu)


# ------------------------------------------------------------------------------------------------ AdamW
@pytest.mark.parametrize("step0", [1, 100000])
@pytest.mark.parametrize("wd,gscale,clip", [(0.0, 1.0, None), (0.1, 0.125, 1e9), (0.1, 1.0, 0.5)])
def test_adamw_faithful_passes(step0, wd, gscale, clip):
    n = 1023
    p, g = rnd((n,), 40, 1.0, F32), rnd((n,), 41, 0.1)
    g[:3] = 0
    m, v = torch.zeros(n), torch.zeros(n)
    ref = R.AdamW64(p, m, v, 1e-3, 0.9, 0.999, 1e-8, wd)
    sq = g.float().pow(2).sum().item() if clip is not None else None
    for t in range(step0, step0 + 4):
        p, m, v, w = adamw(p, m, v, g, 1e-3, 0.9, 0.999, 1e-8, wd, t, gscale, sq, clip or 0.0)
        ref.step(g, t, gscale, sq, clip or 0.0).check(f"host adamw", p, m, v, w)


@pytest.mark.parametrize("fault", ["no_bc2", "wd_new"])
def test_adamw_fault_is_caught(fault):
    n = 1023
    p, g = rnd((n,), 40, 1.0, F32), rnd((n,), 41, 0.1)
    ref = R.AdamW64(p, torch.zeros(n), torch.zeros(n), 1e-3, 0.9, 0.999, 1e-8, 0.1)
    p, m, v, w = adamw(p, torch.zeros(n), torch.zeros(n), g, 1e-3, 0.9, 0.999, 1e-8, 0.1, 1, fault=fault)
    with pytest.raises(AssertionError, match="fault p: "):
        ref.step(g, 1).check("fault", p, m, v, w)


def test_print_ratio_table():
    """Runs last in this file: the largest ratio of every check family above (`pytest -s`)."""
    fam = {}
    for k, r in R.RATIOS.items():
        if k.startswith("host"):
            fam[k] = r
    for k in sorted(fam):
        print(f"\nRATIO {k}: {fam[k]:.3f}", end="")
    assert all(r <= 1 for r in fam.values())
