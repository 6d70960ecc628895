"""tests/vision_ref.py proven on the host: every fp64 restatement against torch's own operator in fp64 where one exists, every checker
shown to accept a faithful stand-in (the restatement with the kernel's rounding points applied in torch) and to reject planted faults:
one element off by one bf16 ulp, a P row normalised without one lane group's share of the sum, a mask index shifted by one, the
rotate-half sign flipped for one 16-feature block, a tie rounded away from even, a causal limit off by one. No GPU."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import vision_ref as V
from tests.rowwise_ref import BF16, F32, F64, E, bf


def randn(shape, seed, scale=1.0, dtype=F64):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=F64) * scale).to(dtype)


def ulp_up(t, idx):
    """t (bf16) with element idx moved to the next bf16 value away from zero."""
    t = t.clone()
    v = t.view(-1).view(torch.int16)
    v[idx] += 1
    return t


# ================================================================================================ dropout hash
def test_hash_by_hand():
    """The three values of drop_bits_int's docstring with their intermediate z, worked from the formula with Python integers."""
    M = (1 << 64) - 1
    cases = [(0, 0, 0x9E3779B97F4A7C15, 0x6F68261B57E7A770, 0xE220A838BF5C9DDE, 14819496),
             (1, 1 << 32, 0x1D81F5CE7F4A7C16, 0x7204A41FCD1DBFF7, 0x16C3E97692A50EDA, 1491945),
             (M, (1 << 40) + 5, 0xFFC8EF58FBBEE87D, 0xF5CB451C298E58AE, 0x2CB5213D9EF16B79, 2929953)]
    for seed, idx, z0, z1, z2, bits in cases:
        assert (seed + 0x9E3779B97F4A7C15 * (idx + 1)) & M == z0
        assert ((z0 ^ (z0 >> 30)) * 0xBF58476D1CE4E5B9) & M == z1
        assert ((z1 ^ (z1 >> 27)) * 0x94D049BB133111EB) & M == z2
        assert (z2 ^ (z2 >> 31)) >> 40 == bits
        assert V.drop_bits_int(seed, idx) == bits and int(V.drop_bits(seed, [idx])[0]) == bits
    idx = np.random.default_rng(0).integers(0, 2 ** 63, 1000, dtype=np.uint64)
    assert [int(b) for b in V.drop_bits(12345, idx)] == [V.drop_bits_int(12345, int(i)) for i in idx]
    keep = V.drop_keep(7, 2 ** 32 - 3, 100000, 0.25)
    assert abs(keep.float().mean().item() - 0.75) < 0.01
    assert V.drop_params(0.25) == (4194304, float(np.float32(1) / np.float32(0.75)))
    x = randn((64,), 1, 1.0, BF16)
    y = V.dropout_ref(x, keep[:64], 0.25)
    assert torch.equal(y[keep[:64]], (x.float() * float(np.float32(1) / np.float32(0.75))).to(BF16)[keep[:64]]) and (y[~keep[:64]] == 0).all()


# ================================================================================================ softmax, cross-attention
def test_softmax64_and_causal():
    S = randn((3, 5, 9), 2, 3.0)
    assert torch.allclose(V.softmax64(S), torch.softmax(S, -1), rtol=1e-14, atol=0)
    al = V.causal_allowed(5, 9, "cpu")
    assert torch.equal(al, torch.ones(5, 9, dtype=torch.bool).tril())
    assert torch.equal(V.causal_allowed(9, 5, "cpu"), torch.ones(9, 5, dtype=torch.bool).tril())
    ref = torch.softmax(S.masked_fill(~al, -float("inf")), -1)
    assert torch.allclose(V.softmax64(S, al.expand(3, 5, 9)), ref, rtol=1e-14, atol=0)
    none = torch.zeros(3, 5, 9, dtype=torch.bool)
    assert (V.softmax64(S, none) == 0).all()


def softmax_standin(S, allowed, Lk, ldP):
    P = torch.zeros((*S.shape[:-1], ldP), dtype=BF16)
    P[..., :Lk] = V.softmax64(S[..., :Lk], allowed).to(F32).to(BF16)
    return P


def test_softmax_checkers_accept_and_reject():
    nb, Lq, Lk = 2, 7, 70
    S = randn((nb, Lq, Lk + 3), 3, 2.0, F32)
    al = V.causal_allowed(Lq, Lk, "cpu")[None].expand(nb, Lq, Lk)
    P = softmax_standin(S, al, Lk, Lk + 5)
    V.check_softmax_fwd("host softmax", P, S, al, Lk)
    with pytest.raises(AssertionError):                 # one element off by one bf16 ulp
        V.check_softmax_fwd("host softmax", ulp_up(P, 3 * (Lk + 5) + 1), S, al, Lk)
    with pytest.raises(AssertionError):                 # a causal limit off by one
        V.check_softmax_fwd("host softmax", softmax_standin(S, torch.ones(Lq, Lk, dtype=torch.bool).tril(-1)[None].expand(nb, Lq, Lk), Lk, Lk + 5),
                            S, al, Lk)
    with pytest.raises(AssertionError):                 # a pad column that is not zero
        Q = P.clone(); Q[0, 0, Lk + 1] = 1e-3
        V.check_softmax_fwd("host softmax", Q, S, al, Lk)
    dP = randn((nb, Lq, Lk + 3), 4, 1.0, F32)
    p, g = P[..., :Lk].double(), dP[..., :Lk].double()
    dS = torch.zeros_like(P)
    dS[..., :Lk] = (0.125 * p * (g - (p * g).sum(-1, keepdim=True))).to(F32).to(BF16)
    V.check_softmax_bwd("host softmax_bwd", dS, P, dP, Lk, 0.125)
    with pytest.raises(AssertionError):
        V.check_softmax_bwd("host softmax_bwd", ulp_up(dS, 5 * (Lk + 5) + 2), P, dP, Lk, 0.125)
    with pytest.raises(AssertionError):                 # the row dot left out
        bad = dS.clone(); bad[..., :Lk] = (0.125 * p * g).to(BF16)
        V.check_softmax_bwd("host softmax_bwd", bad, P, dP, Lk, 0.125)


def xattn_standin(q, k, v, alpha, T, Tp, p_drop, seed, offset, lose_group=None, shift=0):
    B, N, H, hd = q.shape
    S, _, Vv = V.xattn_parts(q, k, v, alpha)
    p = V.softmax64(S)
    if lose_group is not None:                          # the sum without lane group g's keys (4 g + r of every 16-key tile)
        ex = (S - S.amax(-1, keepdim=True)).exp()
        grp = (torch.arange(T) % 16) // 4 == lose_group
        p = ex / ex[..., ~grp].sum(-1, keepdim=True)
    P = torch.zeros((B * H, N, Tp), dtype=BF16)
    P[..., :T] = p.reshape(B * H, N, T).to(F32).to(BF16)
    Pd = P
    if p_drop:
        Pd = V.dropout_ref(P, V.drop_keep(seed, offset + shift, P.numel(), p_drop), p_drop)
    o = (Pd.view(B, H, N, Tp)[..., :T].double() @ Vv).to(F32).to(BF16).permute(0, 2, 1, 3)
    return o, P, Pd


@pytest.mark.parametrize("T,Tp,p_drop", [(40, 64, 0.0), (150, 152, 0.25)])
def test_xattn_checker_accepts_and_rejects(T, Tp, p_drop):
    B, N, H, hd = 2, 5, 2, 64
    q, k, v = randn((B, N, H, hd), 5, 1.0, BF16), randn((B, T, H, hd), 6, 1.0, BF16), randn((B, T, H, hd), 7, 1.0, BF16)
    alpha, seed, off = hd ** -0.5, 99, 2 ** 32 - 5
    # the restatement against torch's own attention
    S, _, Vv = V.xattn_parts(q, k, v, alpha)
    sd = F.scaled_dot_product_attention(q.double().permute(0, 2, 1, 3), k.double().permute(0, 2, 1, 3), v.double().permute(0, 2, 1, 3), scale=alpha)
    assert torch.allclose(V.softmax64(S) @ Vv, sd, rtol=1e-12, atol=1e-14)
    o, P, Pd = xattn_standin(q, k, v, alpha, T, Tp, p_drop, seed, off)
    V.check_xattn("host xattn", o, P, Pd, q, k, v, alpha, T, Tp, p_drop, seed, off)
    V.check_xattn("host xattn", o, None, None, q, k, v, alpha, T, Tp, p_drop, seed, off)
    with pytest.raises(AssertionError):                 # one element of O off by one bf16 ulp
        V.check_xattn("host xattn", ulp_up(o.contiguous(), 77), P, Pd, q, k, v, alpha, T, Tp, p_drop, seed, off)
    with pytest.raises(AssertionError):                 # a row normalised without one lane group's share of the sum
        V.check_xattn("host xattn", *xattn_standin(q, k, v, alpha, T, Tp, p_drop, seed, off, lose_group=2), q, k, v, alpha, T, Tp, p_drop, seed, off)
    if p_drop:
        with pytest.raises(AssertionError):             # a mask index shifted by one
            V.check_xattn("host xattn", *xattn_standin(q, k, v, alpha, T, Tp, p_drop, seed, off, shift=1), q, k, v, alpha, T, Tp, p_drop, seed, off)


# ================================================================================================ GELU
def test_gelu_restatement_and_fit_figures():
    x = randn((4096,), 8, 2.5)
    assert torch.allclose(V.gelu64(x), F.gelu(x), rtol=1e-12, atol=1e-15)
    xa = x.clone().requires_grad_(True)
    F.gelu(xa).sum().backward()
    cdf, zpdf = V.gelu_dgelu64(x)
    assert torch.allclose(cdf + zpdf, xa.grad, rtol=1e-12, atol=1e-15)
    assert abs(V.gelu64(torch.tensor([-10.0])).item() / (-10 * 0.5 * math.erfc(10 / math.sqrt(2))) - 1) < 1e-12      # the tail keeps its relative accuracy
    b = V.gelu_fit_error(V.GELU_B_COEF)
    assert 2.50e-4 < b["rel"] < 2.52e-4 and 0.0640 < b["rel_ulp"] < 0.0645 and 3.3e-5 < b["abs"] < 3.45e-5 and 1.04e-7 < b["far"] < 1.05e-7
    assert b["rel"] + 5 * 26 * E * math.log(2) < 2.6e-4 and b["far"] < 1.1e-7                # the bf16 form's bound e
    fit, total = V.gelu7_tail_rel()
    assert 4.2e-6 < fit < 4.3e-6 and total < 1.2e-5
    assert abs(V.GELU_FAR - 1.0444e-7) < 1e-11


def gelu7_f32(x, old):
    """The f32 form evaluated in torch float32 on the host: the construction before this restatement existed (phi = 0.5 + copysign(0.5 - 2^q, x),
    GELU = x phi) and the present one (relu(x) - a 2^q)."""
    x = x.to(F32)
    a = x.abs().clamp_max(5.5)
    q = torch.full_like(a, V.GELU_7_COEF[0])
    for c in V.GELU_7_COEF[1:]:
        q = (q.double() * a.double() + c).to(F32)         # fma: one rounding
    e = torch.exp2(q.double()).to(F32)
    if old:
        return x * (0.5 + torch.copysign(0.5 - e, x))
    return ((x - x.clamp_max(0)).double() - a.double() * e.double()).to(F32)


def test_gelu_checkers_accept_and_reject():
    z = V.all_bf16()
    h = V.gelu_fit(z, V.GELU_B_COEF).to(F32).to(BF16)
    V.check_gelu_b("host gelu_b", h, z)
    with pytest.raises(AssertionError):
        V.check_gelu_b("host gelu_b", ulp_up(h, 0x4000), z)                                  # GELU(2.0) one ulp up
    V.check_gelu_f32("host gelu f32", gelu7_f32(z, old=False), z)
    old = gelu7_f32(z, old=True)
    assert abs(old[0xC0A0].item() / -1.4901e-6 - 1) < 1e-3 and abs(V.gelu64(z[0xC0A0:0xC0A1]).item() / -1.4333e-6 - 1) < 1e-3     # GELU(-5): 4 % off
    assert old[0xC974].item() < -0.02                         # x 2^-25 below -5.5: -0.03 at -1e6
    with pytest.raises(AssertionError):
        V.check_gelu_f32("host gelu f32 (old form)", old, z)
    dh = torch.tensor([1.0, -3.0, 2.0 ** -100, 3e38]).to(BF16).repeat_interleave(65536)
    zz = z.repeat(4)
    cdf, zpdf = V.gelu_dgelu64(zz)
    dz = (dh.double() * (cdf + zpdf)).to(F32).to(BF16)
    fin = V.check_gelu_bwd("host gelu_bwd", dz, dh, zz)
    assert fin.all()                                     # (3e38 times the largest slope, 1.13, is still inside bf16)
    with pytest.raises(AssertionError):
        V.check_gelu_bwd("host gelu_bwd", ulp_up(dz, 0x3F80), dh, zz)


# ================================================================================================ ViT q/k-prep, im2col
def vit_standin(qkv, N, NH, qn, kn, cos, sin, P, ps, Wp, eps, flip_block=None):
    xq, xk, xv = V.vit_split(qkv, N, NH)
    out = []
    for x, nw in ((xq, qn), (xk, kn)):
        n = x.double()
        if nw is not None:
            n = F.layer_norm(n, (64,), nw[0].double(), nw[1].double(), eps).to(F32).to(BF16).double()
        if cos is not None:
            if flip_block is not None:                  # the rotate-half sign of one 16-feature block flipped
                py, px = V.vit_positions(N, P, ps, Wp, "cpu")
                c = torch.cat([cos.double()[py], cos.double()[px]], -1)
                s = torch.cat([sin.double()[py], sin.double()[px]], -1)
                r = V.rot_half32(n)
                r[..., 16 * flip_block:16 * flip_block + 16] *= -1
                n = V.rbf32(bf(n * c) + bf(r * s))
            else:
                n = V.vit_rope64(n, cos, sin, N, P, ps, Wp, rounded=True)
        out.append(n.to(BF16).contiguous())
    return out[0], out[1], xv.contiguous()


def test_vit_qkprep_checker_accepts_and_rejects():
    G, NH, Hp, Wp, ps, eps = 2, 4, 3, 4, 5, 1e-5
    P = ps + Hp * Wp
    N = 3 * P
    qkv = randn((G * N, 3 * NH * 64), 9, 1.0, BF16)
    qkv[2::5] = (100 + 0.1 * qkv[2::5].float()).to(BF16)
    qn = (torch.rand(64) + 0.5, randn((64,), 10, 0.1, F32))
    kn = (torch.rand(64) + 0.5, randn((64,), 11, 0.1, F32))
    ang = torch.rand(5, 16) * 3
    cos, sin = torch.cat([ang, ang], -1).cos().to(BF16), torch.cat([ang, ang], -1).sin().to(BF16)
    # LayerNorm restatement against torch's own
    v, _ = V.vit_norm64(qkv.view(-1, 64), qn[0], qn[1], eps, 4, 4)
    assert torch.allclose(v, F.layer_norm(qkv.view(-1, 64).double(), (64,), qn[0].double(), qn[1].double(), eps), rtol=1e-9, atol=1e-9)
    # rotate-half: feature e takes -x[e + 16] in the lower half of its 32-block, x[e - 16] in the upper
    t = torch.arange(64.0).double()
    assert torch.equal(V.rot_half32(t), torch.cat([-t[16:32], t[:16], -t[48:], t[32:48]]))
    py, px = V.vit_positions(N, P, ps, Wp, "cpu")
    assert py[:ps].tolist() == [0] * ps and (py[ps], px[ps]) == (1, 1) and (py[P - 1], px[P - 1]) == (Hp, Wp) and py[P + ps] == 1
    for use_norm, use_rope in ((True, True), (True, False), (False, True), (False, False)):
        a = (qn if use_norm else None, kn if use_norm else None, cos if use_rope else None, sin if use_rope else None)
        Q, K, Vv = vit_standin(qkv, N, NH, *a, P, ps, Wp, eps)
        for layout in (4, 2):
            V.check_vit_qkprep("host vit_qkprep", Q, K, Vv, qkv, N, NH, *a, P, ps, Wp, eps, layout)
        if use_norm or use_rope:
            with pytest.raises(AssertionError):
                V.check_vit_qkprep("host vit_qkprep", ulp_up(Q, 64 * 3 + 5), K, Vv, qkv, N, NH, *a, P, ps, Wp, eps, 4)
        if use_rope:
            with pytest.raises(AssertionError):
                V.check_vit_qkprep("host vit_qkprep", *vit_standin(qkv, N, NH, *a, P, ps, Wp, eps, flip_block=2), qkv, N, NH, *a, P, ps, Wp, eps, 4)


def test_im2col_restatement():
    p, Kp, NI, H, W = 2, 16, 2, 4, 6
    img = torch.rand(NI, 3, H, W)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    cands = V.im2col64(img, p, Kp, mean, std)
    m = torch.tensor(mean).to(BF16).float().view(1, 3, 1, 1)
    s = torch.tensor(std).to(BF16).float().view(1, 3, 1, 1)
    norm = ((img.to(BF16).float() - m).to(BF16).float() / s).to(BF16)
    ref = F.unfold(norm.float(), kernel_size=p, stride=p).transpose(1, 2).reshape(-1, 3 * p * p)         # [NI Hp Wp, 3 p p]
    assert torch.equal(cands[0][:, :12].float(), ref) and (cands[0][:, 12:] == 0).all()
    assert all(torch.equal(c, cands[0]) for c in cands[1:])


# ================================================================================================ casts
def test_cast_edges_round_to_nearest_even():
    """torch's CPU conversion, which the GPU test compares with, is round-to-nearest-even on every edge pattern; a tie rounded away
    from even differs from it."""
    e = V.cast_edges()
    u = e.numpy().view(np.uint32).astype(np.uint64)
    want = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    away = ((u + 0x8000) >> 16).astype(np.uint16)
    got = e.view(F32).to(BF16).view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(e.view(F32).numpy())
    assert (got[~nan] == want[~nan]).all() and (got[~nan] != away[~nan]).any()
    assert np.isnan(e.view(F32).to(BF16).float().numpy()[nan]).all() and nan.sum() >= 6
    ties = (u & 0xFFFF) == 0x8000
    assert ties.sum() >= 65536 and ((want[ties & ~nan] & 1) == 0).all()
    assert np.isinf(e.view(F32).to(BF16).float().numpy()[u == 0x7F7FFFFF]).all()            # the largest finite f32 rounds to inf
