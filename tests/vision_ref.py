"""Plain fp64 restatements of the Perceiver- and ViT-side kernels (fused cross-attention, masked softmax and its backward, GELU, the
tower's q/k-prep and im2col, dropout), and the checkers that compare a result with them. Same conventions as tests/rowwise_ref.py, whose
symbols (U, E, TINY, bf, ulp, report, once, among, bits_equal) are used here: every function is written from the formula in torch fp64
on whatever device its operands live on and shares nothing with the kernels; every result is checked tight (the kernel's documented
rounding points applied: `once` for a value rounded once, `among` / an interval of candidates for a value behind two roundings) and
loose (the unrounded function, first-order bound scaled by the sum of the absolute values of the terms), per element or per row.

Error constants used below (each derived where it is used):
  __expf(x): relative (1.45 |x| + 2) E - the argument is scaled by log2(e) in f32 (absolute E |x| log2(e) on the exponent, which 2^x turns
    into 1.45 |x| E relative... to first order) and v_exp_f32 is good to one ulp = 2 E;
  v_rcp_f32, v_rsq_f32: one ulp = 2 E; a correctly rounded f32 operation: E;
  a sum of n f32 terms along chains of `depth` additions: depth E sum|terms|; an MFMA dot product of depth n: (n - 1) E sum|terms|;
  erff (OCML, gelu_bwd_kernel only): ERFF_REL, measured - see there."""
import math

import numpy as np
import torch

from tests.rowwise_ref import BF16, E, F32, F64, TINY, U, bf, bits_equal, once, report, ulp

# ================================================================================================ dropout hash
PHI64 = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1


def drop_bits_int(seed, idx):
    """The definition, in Python integers (csrc/common.h: drop_bits): the splitmix64 finaliser of seed + phi64 (idx + 1), top 24 bits.
        z = seed + 0x9E3779B97F4A7C15 (idx + 1)      (mod 2^64 throughout)
        z = (z ^ (z >> 30)) 0xBF58476D1CE4E5B9
        z = (z ^ (z >> 27)) 0x94D049BB133111EB
        bits = (z ^ (z >> 31)) >> 40
    Three values by hand (tests/test_vision_ref_host.py holds the intermediate z of each):
        (seed 0, idx 0) -> 14819496      (seed 1, idx 2^32) -> 1491945      (seed 2^64 - 1, idx 2^40 + 5) -> 2929953"""
    z = (seed + PHI64 * (idx + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return (z ^ (z >> 31)) >> 40


def drop_bits(seed, idx):
    """The same in numpy uint64 (wrapping arithmetic) for an array of element indices."""
    with np.errstate(over="ignore"):
        idx = np.asarray(idx, dtype=np.uint64)
        z = np.uint64(seed & M64) + np.uint64(PHI64) * (idx + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return ((z ^ (z >> np.uint64(31))) >> np.uint64(40)).astype(np.uint32)


def drop_params(p):
    """(threshold, scale) as the C entries form them from the f32 argument p: (unsigned)(p * 2^24) and 1 / (1 - p), both in f32."""
    p32 = np.float32(p)
    return int(p32 * np.float32(16777216.0)), float(np.float32(1.0) / (np.float32(1.0) - p32))


def drop_keep(seed, offset, n, p, device="cpu"):
    """bool [n]: element i is kept iff drop_bits(seed, offset + i) >= (unsigned)(p 2^24) (64-bit index arithmetic, wrapping)."""
    thresh, _ = drop_params(p)
    with np.errstate(over="ignore"):
        idx = np.uint64(offset & M64) + np.arange(n, dtype=np.uint64)
    return torch.from_numpy(drop_bits(seed, idx) >= np.uint32(thresh)).to(device)


def dropout_ref(x, keep, p):
    """Inverted dropout of a bf16 / f32 tensor, exactly: a kept element is x * scale as ONE f32 product (the fp64 product of a value of at
    most 24 bits and an f32 is exact, so rounding it to f32 is the correctly rounded f32 product), then rounded to the tensor's type."""
    _, scale = drop_params(p)
    y = (x.to(F64) * scale).to(F32).to(x.dtype)
    return torch.where(keep.view(x.shape), y, torch.zeros_like(y))


# ================================================================================================ softmax
def softmax64(S, allowed=None):
    """softmax over the last axis of the allowed entries; a row with none allowed is all zeros."""
    S = S.to(F64)
    if allowed is None:
        allowed = torch.ones_like(S, dtype=torch.bool)
    m = torch.where(allowed, S, torch.full_like(S, -float("inf"))).amax(-1, keepdim=True)
    ex = torch.where(allowed, (S - torch.where(torch.isfinite(m), m, torch.zeros_like(m))).exp(), torch.zeros_like(S))
    tot = ex.sum(-1, keepdim=True)
    return torch.where(tot > 0, ex / tot.clamp_min(1e-300), torch.zeros_like(ex))


def causal_allowed(Lq, Lk, device):
    """Row i of a causal block sees keys 0 .. min(i, Lk - 1) (vq3_softmax_fwd: lim = min(i + 1, Lk), also when Lq != Lk)."""
    return torch.arange(Lk, device=device)[None, :] <= torch.arange(Lq, device=device)[:, None]


def softmax_err(S, allowed, dscore, depth, extra_sum_rel=0.0):
    """(p, e): fp64 softmax and the f32 error bound of exp(s - max) / sum before its one rounding. A score that arrives with absolute
    error ds (dscore; the subtraction of the maximum adds E |s - max|) moves its own exponential by ds relative and the sum by the
    p-weighted mean of the ds; __expf adds (1.45 |s - max| + 2) E; the sum of positive terms along chains of `depth` additions depth E
    (+ extra_sum_rel: what a running rescale adds), the division and the product one E each. Flushed exponentials: TINY."""
    p = softmax64(S, allowed)
    S = S.to(F64)
    m = torch.where(allowed, S, torch.full_like(S, -float("inf"))).amax(-1, keepdim=True)
    d = torch.where(allowed, (S - m).abs(), torch.zeros_like(S))
    r = torch.where(allowed, dscore + E * d + (1.45 * d + 2) * E, torch.zeros_like(S))
    rs = (p * r).sum(-1, keepdim=True)
    return p, p * (r + rs + (depth + 2) * E + extra_sum_rel) + TINY


def check_probs(tag, P, Lk, p, e):
    """P bf16 [..., ldP] against (p, e) [..., Lk]: tight per element, every row sums to 1 (or 0) within the sum of its elements' bounds,
    pad columns exactly zero; loose: U p + e."""
    got = P[..., :Lk].to(F64)
    assert (P[..., Lk:] == 0).all(), tag + ": pad columns must be exactly zero"
    once(tag + " P tight", got, p, e)
    report(tag + " P loose", (got - p).abs(), U * p + e)
    report(tag + " P row sum", (got.sum(-1) - p.sum(-1)).abs(), (ulp(p + e) / 2 + e).sum(-1))


def check_softmax_fwd(tag, P, S, allowed, Lk):
    """vq3_softmax_fwd: one wave per row, a lane adds ceil(Lk / 64) exponentials, 6 butterfly levels; the scores are the kernel's own input."""
    p, e = softmax_err(S[..., :Lk], allowed, 0.0, math.ceil(Lk / 64) + 6)
    check_probs(tag, P, Lk, p, e)
    return p


def check_softmax_bwd(tag, dS, P, dP, Lk, scale):
    """dS = bf16(scale P (dP - sum P dP)) from the kernel's own bf16 P. The row dot adds ceil(Lk / 64) products per lane and 6 levels; the
    difference cancels, so the bound scales by |P| (|dP| + sum|P dP|): the dot (depth + 1) E sum|P dP|, the subtraction and the two
    products 3 E. scale arrives as an f32."""
    assert (dS[..., Lk:] == 0).all(), tag + ": pad columns must be exactly zero"
    p, g = P[..., :Lk].to(F64), dP[..., :Lk].to(F64)
    sc = float(np.float32(scale))
    dot, adot = (p * g).sum(-1, keepdim=True), (p * g).abs().sum(-1, keepdim=True)
    ref = sc * p * (g - dot)
    depth = math.ceil(Lk / 64) + 6
    e = abs(sc) * p * ((depth + 1) * E * adot + 3 * E * (g.abs() + dot.abs())) + TINY
    once(tag + " dS tight", dS[..., :Lk], ref, e)
    report(tag + " dS loose", (dS[..., :Lk].to(F64) - ref).abs(), U * ref.abs() + e)


# ================================================================================================ fused Perceiver cross-attention
def xattn_parts(q, k, v, alpha):
    """q [B, N, H, hd], k / v [B, T, H, hd] (views of the operands the kernel reads) -> S = alpha q k^T [B, H, N, T], sum|alpha q k|
    (what the score's accumulation error scales by), V [B, H, T, hd] - fp64."""
    q64, k64 = q.to(F64).permute(0, 2, 1, 3), k.to(F64).permute(0, 2, 1, 3)
    a = float(np.float32(alpha))
    S = a * (q64 @ k64.transpose(-1, -2))
    aS = abs(a) * (q64.abs() @ k64.abs().transpose(-1, -2))
    return S, aS, v.to(F64).permute(0, 2, 1, 3)


def check_xattn(tag, o, P, Pd, q, k, v, alpha, T, Tp, p_drop, seed, offset):
    """o bf16 [B, N, H, hd] (a view), P / Pd bf16 [B H, N, Tp] or None. The score: an MFMA dot product of depth hd ((hd - 1) E sum|q k|),
    times alpha (E), minus the maximum (E, in softmax_err). T <= 128: a lane adds 32 exponentials and two levels join the four lane groups
    (depth 34); beyond: 8 per 32-key chunk, + 1 for the running sum, and at most one rescale l * __expf(m - mn) per chunk and the final one,
    each (1.45 R + 3) E with R the row's score range."""
    B, N, H, hd = q.shape
    S, aS, V = xattn_parts(q, k, v, alpha)
    nck = math.ceil(T / 32)
    allowed = torch.ones_like(S, dtype=torch.bool)
    if T <= 128:
        depth, extra = 34, 0.0
    else:
        R = (S.amax(-1, keepdim=True) - S.amin(-1, keepdim=True))
        depth, extra = 9 * nck + 3, (nck + 1) * (1.45 * R + 3) * E
    p, e = softmax_err(S, allowed, (hd - 1) * E * aS + 2 * E * S.abs(), depth, extra)
    assert torch.isfinite(bf(p)).all()
    thresh, scale = drop_params(p_drop)
    keep = torch.ones_like(p, dtype=torch.bool)
    if thresh:
        keep = drop_keep(seed, offset, B * H * N * Tp, p_drop, p.device).view(B, H, N, Tp)[..., :T]
    if P is not None:
        check_probs(tag, P.view(B, H, N, Tp), T, p, e)
    if Pd is not None:
        assert P is not None
        want = P if not thresh else dropout_ref(P, drop_keep(seed, offset, P.numel(), p_drop, P.device), p_drop)
        assert bits_equal(Pd, want), tag + ": Pd must be the restated dropout of the kernel's own P, bit for bit"
    got = o.to(F64).permute(0, 2, 1, 3)                                        # [B, H, N, hd]
    kern_pd = (Pd if Pd is not None else P)
    if kern_pd is not None:
        # tight: the kernel's own bf16 weights times V: an MFMA accumulation over the 32 nck visited keys, one rounding
        w = kern_pd.view(B, H, N, Tp)[..., :T].to(F64)
        ref = w @ V
        once(tag + " O tight", got, ref, (32 * nck - 1) * E * (w.abs() @ V.abs()) + TINY)
    # loose: the whole function. A weight is bf16(bf16(p (1 +- e)) scale): |d pd| <= scale (2 U p + e) (1 + U) to first order
    sc = scale if thresh else 1.0
    pd = torch.where(keep, p * sc, torch.zeros_like(p))
    dpd = torch.where(keep, sc * ((2 * U + U * U) * p + e * (1 + 2 * U)), torch.zeros_like(p)) if thresh else U * p + e
    ref = pd @ V
    mag = pd @ V.abs()
    report(tag + " O loose", (got - ref).abs(), dpd @ V.abs() + (32 * nck - 1) * E * mag + U * ref.abs() + TINY)
    return p


# ================================================================================================ GELU
# the kernels' published coefficients (csrc/common.h), highest degree first: q(a) ~ log2 Phi(-a) on [0, 5.5]
GELU_B_COEF = (-2.3323995992541313e-04, 4.869441967457533e-03, -4.4596340507268906e-02, -4.6968939900398254e-01, -1.1462510824203491e+00,
               -1.0003620386123657e+00)
GELU_7_COEF = (-1.921234625e-06, 6.328849712e-05, -9.434208502e-04, 8.556272268e-03, -5.405228293e-02, -4.583817849e-01, -1.151278331e+00,
               -9.999938561e-01)
GELU_CLAMP = 5.5
GELU_FAR = 5.5 * 0.5 * math.erfc(5.5 / math.sqrt(2.0))          # 5.5 Phi(-5.5) = 1.0444e-7: what both forms return (negated) below -5.5


def gelu64(x):
    """x Phi(x), Phi through erfc so that the negative tail keeps its relative accuracy."""
    x = x.to(F64)
    return x * 0.5 * torch.erfc(-x / math.sqrt(2.0))


def gelu_dgelu64(z):
    """d/dz (z Phi(z)) = Phi(z) + z phi(z), and the two terms."""
    z = z.to(F64)
    cdf = 0.5 * torch.erfc(-z / math.sqrt(2.0))
    return cdf, z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def all_bf16(device="cpu", normal_only=True):
    """Every bf16 bit pattern as a bf16 tensor [65536]; normal_only: the finite normal values and +-0 (the others replaced by 0)."""
    x = torch.arange(65536, dtype=torch.int32, device=device).to(torch.int16).view(BF16)
    if normal_only:
        xf = x.to(F64)
        ok = torch.isfinite(xf) & ((xf.abs() >= TINY) | (xf == 0))
        x = torch.where(ok, x, torch.zeros_like(x))
    return x


def gelu_fit(x, coef):
    """The kernels' construction with the published coefficients, evaluated in fp64: relu(x) - a 2^q(a), a = min(|x|, 5.5)."""
    x = x.to(F64)
    a = x.abs().clamp_max(GELU_CLAMP)
    q = torch.full_like(a, coef[0])
    for c in coef[1:]:
        q = q * a + c
    return x.clamp_min(0) - a * torch.exp2(q)


def gelu_fit_error(coef):
    """The fit's own error over every finite normal bf16 argument: worst relative and absolute error on |x| < 5.5, the largest |result|
    and the largest absolute error beyond. bf16 form: 2.51e-4 (0.064 bf16 ulp), 3.4e-5, 1.04e-7. This is where the bf16 form's bound
    e = 2.6e-4 |GELU(x)| + 1.1e-7 comes from: the relative figure with a margin for the f32 evaluation of q (5 roundings at |q| <= 26:
    5 * 26 E ln 2 = 5e-6), and the clamp's constant for the arguments below -5.5, where |GELU| < 1.04e-7 itself."""
    x = all_bf16().to(F64)
    x = x[x != 0]
    fit, ref = gelu_fit(x, coef), gelu64(x)
    near = x.abs() < GELU_CLAMP
    err = (fit - ref).abs()
    return dict(rel=(err / ref.abs())[near].max().item(), abs=err[near].max().item(), rel_ulp=(err / ulp(ref))[near].max().item(),
                far=fit[~near & (x < 0)].abs().max().item(), far_err=err[~near].max().item())


def gelu7_tail_rel():
    """Relative error bound of the f32 form's a 2^q(a) on [0, 5.5], the quantity its negative tail is made of: the degree-7 fit's own error
    against Phi(-a) on a dense grid (4.3e-6), plus q's f32 evaluation - the Horner step that still has k multiplications by a ahead of it
    rounds E |partial| and reaches q as E |partial| a^k, and 2^q turns an absolute dq into ln 2 dq relative (3.4e-6 at a = 5.5) - plus
    v_exp_f32's ulp (2 E) and the product and the final fma (2 E). 7.9e-6 in all, inside the 1.2e-5 the kernel's comment states.
    Returns (the fit's share, the total)."""
    a = torch.linspace(0, GELU_CLAMP, 200001, dtype=F64)
    q, dq = torch.full_like(a, GELU_7_COEF[0]), torch.zeros_like(a)
    for c in GELU_7_COEF[1:]:
        q = q * a + c
        dq = dq * a + E * q.abs()
    fit = (torch.exp2(q) / (0.5 * torch.erfc(a / math.sqrt(2.0))) - 1).abs().max().item()
    return fit, fit + (math.log(2.0) * dq).max().item() + 4 * E


def check_gelu_b(tag, h, z):
    """The bf16 form (vq3_gelu_fwd, a GEMM's bf16 epilogue): bf16(GELU(z)) within ulp / 2 + e, e = 2.6e-4 |GELU(z)| + 1.1e-7."""
    ref = gelu64(z)
    assert torch.isfinite(bf(ref)).all()
    assert torch.isfinite(h.to(F64)).all(), tag + ": non-finite result for a finite argument"
    once(tag + " tight", h, ref, 2.6e-4 * ref.abs() + 1.1e-7)
    report(tag + " loose", (h.to(F64) - ref).abs(), (U + 2.6e-4) * ref.abs() + 1.1e-7)


def check_gelu_f32(tag, y, z):
    """The f32 form (a GEMM's f32 epilogue), against what its comment states: 7e-7 absolute and 1.2e-5 relative on |x| < 3; the relative
    bound on the negative tail down to -5.5; below that |result| <= 5.5 Phi(-5.5) (1 + 1e-3); above 3 the result is x minus a term below
    4.1e-3 that carries the relative bound, rounded once (E |result|). TINY: a result among the f32 denormals."""
    x, got, ref = z.to(F64), y.to(F64), gelu64(z)
    assert torch.isfinite(got).all(), tag + ": non-finite result for a finite argument"
    err = (got - ref).abs()
    m = x.abs() < 3
    report(tag + " |x| < 3 abs", err[m], torch.full_like(err[m], 7e-7))
    report(tag + " |x| < 3 rel", err[m], 1.2e-5 * ref.abs()[m] + TINY)
    m = (x <= -3) & (x >= -GELU_CLAMP)
    report(tag + " negative tail rel", err[m], 1.2e-5 * ref.abs()[m])
    m = x < -GELU_CLAMP
    report(tag + " far tail", got.abs()[m], torch.full_like(err[m], GELU_FAR * (1 + 1e-3)))
    m = x >= 3
    report(tag + " x >= 3", err[m], E * ref.abs()[m] + 1.2e-5 * (x - ref).abs()[m] + GELU_FAR * 1e-3)


# erff of OCML against fp64 erf: the largest relative error of the ROCm build's f32 torch.erf (OCML's erff too, and not the code under
# test) over all 65 278 finite non-zero bf16 arguments, on an MI355X: 6.1812e-06 = 103.7 E, measured 2026-10-19 by
# tests/test_vision_fp64_gpu.py::test_erff_constant, which repeats the measurement on every run and prints where the maximum sits: at
# the denormal argument 9.18e-41 (over the normal arguments alone it is 1.17e-7 = 2 E; z / sqrt 2 is denormal for the smallest normal
# z, so the whole range counts). The constant is twice the figure - the factor covers another OCML revision in torch's build. (It
# reaches Phi as 0.5 ERFF_REL |erf|: 6e-6 absolute at most, against half a bf16 ulp of 2e-3 for a slope near 1.)
ERFF_REL_MEASURED = 6.1812e-06
ERFF_REL = 2 * ERFF_REL_MEASURED


def check_gelu_bwd(tag, dz, dh, z):
    """dz = bf16(dh (Phi(z) + z phi(z))), Phi = 0.5 (1 + erff(z / sqrt 2)), phi = __expf(-z^2 / 2) / sqrt(2 pi), f32 throughout.
    Phi: the argument u = z * f32(1 / sqrt 2) carries 2 E |u|, which erf' = 2 / sqrt(pi) e^(-u^2) turns into an absolute error; erff
    ERFF_REL |erf u|; 1 + erf rounds E |1 + erf| - for z << 0 the f32 sum is 0 where Phi is 1e-10: covered, the bound is absolute.
    phi: w = z^2 / 2 rounds twice (2 E w on the exponent: 2 E w relative), __expf (1.45 w + 2) E, the constant and its product 2 E;
    a flushed exponential TINY. z phi, the sum and the product with dh: E each of the terms."""
    zz, d = z.to(F64), dh.to(F64)
    cdf, zpdf = gelu_dgelu64(z)
    u = zz / math.sqrt(2.0)
    erf = torch.erf(u)
    e_cdf = 0.5 * (ERFF_REL * erf.abs() + 2 * E * u.abs() * 2 / math.sqrt(math.pi) * torch.exp(-u * u) + E * (1 + erf).abs())
    w = 0.5 * zz * zz
    e_zpdf = zpdf.abs() * ((3.45 * w + 4) * E + E) + zz.abs() * TINY
    ref = d * (cdf + zpdf)
    e = d.abs() * (e_cdf + e_zpdf + 2 * E * (cdf.abs() + zpdf.abs())) + TINY
    fin = torch.isfinite(bf(ref))
    got = dz.to(F64)
    assert torch.isfinite(got[fin]).all(), tag + ": non-finite dz where the fp64 result is finite in bf16"
    once(tag + " tight", got[fin], ref[fin], e[fin])
    report(tag + " loose", (got - ref).abs()[fin], (U * ref.abs() + e)[fin])
    return fin


# ================================================================================================ ViT q/k-prep
def vit_positions(N, P, patch_start, Wp, device):
    """(py, px) of token n of a group of N tokens made of frames of P: tokens below patch_start of their frame sit at 0."""
    tp = torch.arange(N, device=device) % P
    z = torch.zeros_like(tp)
    return torch.where(tp >= patch_start, (tp - patch_start) // Wp + 1, z), torch.where(tp >= patch_start, (tp - patch_start) % Wp + 1, z)


def rot_half32(t):
    """rotate-half inside each 32-feature block of the 64: feature e takes -x[e + 16] for (e & 16) == 0, else x[e - 16]."""
    b = t.reshape(*t.shape[:-1], 2, 2, 16)
    return torch.stack([-b[..., 1, :], b[..., 0, :]], -2).reshape(t.shape)


def rbf32(x):
    """fp64 -> f32 -> bf16 -> fp64: a bf16 rounding of an f32 operation's result whose exact value x is."""
    return x.to(F32).to(BF16).to(F64)


def vit_rope64(n, cos, sin, N, P, patch_start, Wp, rounded):
    """2-D RoPE of [G, NH, N, 64]: the first 32 features turn with the patch row, the last 32 with the column. rounded: with the kernel's
    three rounding points, bf16(bf16(x c) + bf16(r s)) - exact arithmetic on bf16 operands; else the unrounded value and |x c| + |r s|."""
    py, px = vit_positions(N, P, patch_start, Wp, n.device)
    c = torch.cat([cos.to(F64)[py], cos.to(F64)[px]], -1)                   # [N, 64]
    s = torch.cat([sin.to(F64)[py], sin.to(F64)[px]], -1)
    r = rot_half32(n)
    if rounded:
        return rbf32(bf(n * c) + bf(r * s))
    return n * c + r * s, (n * c).abs() + (r * s).abs()


def vit_split(qkv, N, NH):
    """qkv [T, 3 NH 64] -> three [G, NH, N, 64] views (q, k, v)."""
    G = qkv.shape[0] // N
    t = qkv.view(G, N, 3, NH, 64).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def vit_norm64(x, w, b, eps, per_lane, levels):
    """Per-head LayerNorm over 64 features: v = d rstd w + b (fp64) and the f32 error of v before its one rounding to bf16.
    A lane adds per_lane values and `levels` butterfly levels join the head (4-feature layout: 4 and 4; 2-feature: 2 and 5), the division
    by 64 is exact: mean carries em = (per_lane - 1 + levels) E mean|x|; d = x - mean: em + E |d|; the variance: 2 mean|d| em for d's
    error, (per_lane + levels + 2) E var for the squares and their sum, E for + eps, TINY-sized squares flush: ev; rstd: ev / (2 (var + eps))
    + 2 E (v_rsq_f32); d * rstd * w + b: 3 E |d rstd w| + E |v|."""
    x64, w64, b64 = x.to(F64), w.to(F64), b.to(F64)
    mean = x64.mean(-1, keepdim=True)
    d = x64 - mean
    var = d.pow(2).mean(-1, keepdim=True)
    rs = torch.rsqrt(var + eps)
    em = (per_lane - 1 + levels) * E * x64.abs().mean(-1, keepdim=True)
    ed = em + E * d.abs()
    ev = 2 * d.abs().mean(-1, keepdim=True) * em + (per_lane + levels + 3) * E * (var + eps) + 64 * TINY
    rrel = ev / (2 * (var + eps)) + 2 * E
    v = d * rs * w64 + b64
    e = ed * (rs * w64).abs() + (rrel + 3 * E) * (d * rs * w64).abs() + E * v.abs() + TINY
    return v, e


def check_vit_qkprep(tag, Q, K, V, qkv, N, NH, qn, kn, cos, sin, P, patch_start, Wp, eps, layout):
    """layout 4 / 2: features per lane. V (and Q, K without norm and rope) bit-exact copies; the normed value must lie between
    bf16(v - e) and bf16(v + e); after RoPE the result is exact given the two normed values it mixes, so it must equal one of the
    candidates built from the ends and the middle of each one's interval."""
    xq, xk, xv = vit_split(qkv, N, NH)
    assert bits_equal(V, xv.contiguous()), tag + ": V must be a bit-exact copy"
    per_lane, levels = (4, 4) if layout == 4 else (2, 5)
    for nm, got, x, nw in (("Q", Q, xq, qn), ("K", K, xk, kn)):
        if nw is None and cos is None:
            assert bits_equal(got, x.contiguous()), f"{tag} {nm}: without norm and rope the head split is a bit-exact copy"
            continue
        got64 = got.to(F64)
        if nw is not None:
            v, e = vit_norm64(x, nw[0], nw[1], eps, per_lane, levels)
            cands = [bf(v - e), bf(v), bf(v + e)]
            loose_n, loose_e = v, (U * v.abs() + e)
        else:
            v = x.to(F64)
            cands, loose_n, loose_e = [v], v, torch.zeros_like(v)
        if cos is None:
            lo, hi = cands[0], cands[-1]
            out = (lo - got64).clamp_min(0) + (got64 - hi).clamp_min(0)
            report(f"{tag} {nm} tight", out, ulp(cands[len(cands) // 2]) / 2)
            report(f"{tag} {nm} loose", (got64 - v).abs(), loose_e + TINY)
            continue
        # the partner's candidate is chosen independently: rotate-half of candidate j for the partner, candidate i for the element itself
        py, px = vit_positions(N, P, patch_start, Wp, v.device)
        c = torch.cat([cos.to(F64)[py], cos.to(F64)[px]], -1)
        s = torch.cat([sin.to(F64)[py], sin.to(F64)[px]], -1)
        # every step (the products, the roundings, the sum) is monotone in each of the two normed values, so the result lies between the
        # smallest and the largest corner; where both intervals are a single bf16 value (nearly everywhere) this is equality
        rc = torch.stack([rbf32(bf(a * c) + bf(rot_half32(b_) * s)) for a in (cands[0], cands[-1]) for b_ in (cands[0], cands[-1])])
        out = (rc.amin(0) - got64).clamp_min(0) + (got64 - rc.amax(0)).clamp_min(0)
        report(f"{tag} {nm} tight", out, ulp(rc[0]) / 2)
        # how much of the tensor is NOT pinned to one value: the rows whose mean error is large against their spread (mean 100 +- 0.1, and
        # the constant rows, whose bound does not know that their sum is exact) - two row kinds in five at the most
        report(f"{tag} {nm} open intervals", (rc.amin(0) != rc.amax(0)).to(F64).mean().reshape(1), torch.full((1,), 0.4, dtype=F64, device=out.device))
        ref, mag = vit_rope64(loose_n, cos, sin, N, P, patch_start, Wp, rounded=False)
        dn = loose_e * c.abs() + rot_half32(loose_e).abs() * s.abs()
        # each product rounds (U), the sum rounds (U): 2 U + U^2 of |x c| + |r s|, plus what the normed values carry
        report(f"{tag} {nm} loose", (got64 - ref).abs(), (2 * U + U * U) * mag + dn * (1 + 2 * U) + TINY)


# ================================================================================================ im2col
def im2col64(img, p, Kp, mean, std):
    """images f32 [NI, 3, H, W] -> candidates for bf16 [NI Hp Wp, Kp]: bf16((bf16(x) - bf16(mean)) / bf16(std)) with a rounding after the
    subtraction, column k = c p^2 + ky p + kx, zero beyond 3 p^2. The difference of two bf16 values is exact in fp64 and its f32-then-bf16
    rounding is taken as the kernel does; the quotient is a correctly rounded f32 division, which the fp64 quotient rounded to f32
    reproduces unless it sits within 2^-50 of an f32 tie - the neighbours at (1 -+ 2^-40) are candidates too."""
    NI, _, H, W = img.shape
    Hp, Wp = H // p, W // p
    m = bf(torch.tensor(mean, dtype=F32, device=img.device).to(F64)).view(1, 3, 1, 1)
    s = bf(torch.tensor(std, dtype=F32, device=img.device).to(F64)).view(1, 3, 1, 1)
    t = rbf32(bf(img.to(F64)) - m)
    out = []
    for f in (1.0, 1 - 2.0 ** -40, 1 + 2.0 ** -40):
        v = rbf32(t / s * f)                                                   # [NI, 3, H, W]
        v = v.view(NI, 3, Hp, p, Wp, p).permute(0, 2, 4, 1, 3, 5).reshape(NI * Hp * Wp, 3 * p * p)
        o = torch.zeros((NI * Hp * Wp, Kp), dtype=F64, device=img.device)
        o[:, :3 * p * p] = v
        out.append(o)
    return out


# ================================================================================================ casts
def cast_edges():
    """f32 bit patterns at which a bf16 conversion can go wrong: ties (low half 0x8000) above an even and an odd upper half at the
    edges of the exponent range, their neighbours 0x7FFF / 0x8001, +-inf, NaNs (among them upper half 0x7F80 with a low payload: truncation
    would make them infinite), the largest finite f32 (rounds to inf), denormals, +-0. int32 tensor; view as f32."""
    hi = [0x0000, 0x0001, 0x0002, 0x007F, 0x0080, 0x0081, 0x3F7F, 0x3F80, 0x3F81, 0x4000, 0x7F7E, 0x7F7F, 0x00FF, 0x0100]
    pats = []
    for h in hi:
        for sgn in (0, 0x8000):
            for lo in (0x0000, 0x7FFF, 0x8000, 0x8001, 0xFFFF, 0x0001):
                pats.append(((h | sgn) << 16) | lo)
    pats += [0x7F800000, 0xFF800000, 0x7F800001, 0xFF800001, 0x7F80FFFF, 0x7FC00000, 0xFFC00000, 0x7FFFFFFF, 0x7F7FFFFF, 0xFF7FFFFF,
             0x00000001, 0x80000001, 0x007FFFFF, 0x00008000, 0x00018000, 0x00000000, 0x80000000]
    up = np.arange(65536, dtype=np.uint32) << 16                              # then EVERY tie, with its two neighbours
    a = np.concatenate([np.array(pats, dtype=np.uint32), up | 0x8000, up | 0x7FFF, up | 0x8001]).view(np.int32)
    return torch.from_numpy(a.copy())
