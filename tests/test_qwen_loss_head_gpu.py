"""The Qwen3 loss head and the tied embedding gradient against a plain fp64 restatement, at the vocabularies the model trains at.

Compared: the cross-entropy kernels (elementwise.hip `cross_entropy_kernel`, both entry points), Qwen3ForCausalLM.loss_head /
backward_loss_head at Qwen3-4B width (gathered rows -> final RMSNorm -> tied lm_head -> cross entropy, and back: the sliced or atomic
lm_head input gradient, dE, the final-norm backward), the embedding / splice backward (`embed_bwd_kernel`, `splice_bwd_kernel`) and the
"live rows" route of VGGTQwen3VLM._backward_text. Every reference runs in fp64 on the device, in vocabulary chunks (no [n, V] fp64
tensor larger than one chunk), from the same bf16 operands the kernels read.

Each comparison is made twice:
  * tight - against fp64 with the kernels' rounding points applied (hn = bf16(w * bf16(x * rstd)), bf16 logits, bf16 dlogits, bf16
    d_hn; a stage is fed the kernel's own bf16 output of the stage before when that output is observable). What is left is f32
    accumulation and a one-ulp flip of a rounded value now and then, so these catch indexing and slicing bugs;
  * loose - against the unrounded fp64 function, with a bound derived next to its constant (first-order propagation of the bf16
    rounding points, computed per row from the reference's own quantities where the sensitivity depends on the row).
Errors are measured per row (per 64-row vocabulary block for dE), never only as a whole-tensor norm; rows whose reference is near 0
get an absolute floor. `pytest -s` prints the largest error / bound ratio of every comparison."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -8          # bf16 unit roundoff: |bf16(x) - x| <= U |x|; one ulp is at most 2 U |x|
VOCAB_VLM = 151670     # the VLM's vocabulary (Qwen3's 151 669 tokens + "<image>"): Vp = 151 680
VOCAB_QWEN = 151936    # Qwen3-4B's own vocabulary: Vp = 151 936
CHUNK = 8192           # fp64 reference chunk over the vocabulary (a multiple of 64: whole dE blocks)


@pytest.fixture(scope="module")
def ops():
    from vggt_qwen3_amd import _lib
    from vggt_qwen3_amd import ops as _ops
    _lib.load()
    return _ops


def bf(x):
    """Round to bf16 and back to fp64 (the kernels' rounding point)."""
    return x.to(BF16).to(F64)


def report(name, err, bound):
    """Assert err <= bound elementwise (per row / block) and print the largest ratio."""
    err, bound = torch.as_tensor(err, dtype=F64), torch.as_tensor(bound, dtype=F64)
    ratio = (err / bound).max().item() if err.numel() else 0.0
    print(f"\nTOL {name}: max err/bound {ratio:.3f} (max err {err.max().item() if err.numel() else 0:.3e})", end="")
    bad = (~(err <= bound)).nonzero().flatten()
    assert bad.numel() == 0, f"{name}: {bad.numel()} rows over bound, first {bad[:8].tolist()}: err {err[bad[:4]].tolist()} " \
                             f"bound {bound.expand_as(err)[bad[:4]].tolist()}"


def lse_err(lse, lmax):
    """Bound on the absolute error of an f32 log-sum-exp (and on the relative error of exp(l - lse)) as the kernel forms it: the sum
    of exponentials is ~150 sequential f32 adds per thread plus a 10-level tree, (160) 2^-24 = 9.5e-6 relative; __expf and __logf
    add about 2^-21 each; mx + log(sum) and l - lse round at 2^-24 of their magnitude."""
    return 1.2e-5 + 2.0 ** -23 * (lse.abs() + lmax)


# ================================================================================================ A. cross-entropy kernels
CE_SHAPES = [(151670, 151680), (151936, 151936), (1000, 1024), (9, 16), (8, 8)]


def ce_case(V, ldl, seed):
    """12 rows: std 1 (rows 0-3), std 8 (4-7), peaked (8-11: the target 20-30 above the rest, loss close to 0); targets at column 0,
    at V - 1, at the row's maximum and random. The slack columns [V, ldl) hold NaN / +inf / -inf; rows n..n8 hold a sentinel."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    n, n8 = 12, 16
    lg = torch.randn(n, V, generator=g, device="cuda", dtype=F64)
    lg[4:8] *= 8
    lg = bf(lg)
    tgt = torch.randint(0, V, (n,), generator=g, device="cuda")
    tgt[[0, 4, 8]] = 0
    tgt[[1, 5, 9]] = V - 1
    tgt[2], tgt[6] = lg[2].argmax(), lg[6].argmax()
    for r in range(8, 12):
        lg[r, tgt[r]] = bf(lg[r].max() + 20 + 10 * torch.rand((), generator=g, device="cuda", dtype=F64))
    buf = torch.randn(n8, ldl, generator=g, device="cuda").to(BF16)   # rows n..n8: sentinel
    buf[:n, :V] = lg.to(BF16)
    if ldl > V:
        slack = torch.tensor([float("nan"), float("inf"), float("-inf")], device="cuda").repeat((ldl - V + 2) // 3)[: ldl - V]
        buf[:n, V:] = slack.to(BF16)
    return n, lg, tgt, buf


def ce_ref(lg, tgt, scale):
    """fp64: lse, per-row loss, p and dlogits = (p - onehot) * scale."""
    lse = torch.logsumexp(lg, 1)
    p = torch.exp(lg - lse[:, None])
    g = p.clone()
    g[torch.arange(lg.shape[0]), tgt] -= 1
    return lse, lse - lg.gather(1, tgt[:, None]).squeeze(1), p, g * scale[:, None]


def check_dlogits(name, got, lg, tgt, scale, lse, p, g):
    """Tight: every element within one ulp of bf16(g) plus the f32 error of p (elementwise, so one wrong column shows). Loose: per row
    ||got - g|| <= U ||g|| (the output rounding) + scale (E ||p|| + 2^-23) (the f32 error of p and of p - 1 at the target)."""
    E = lse_err(lse, lg.abs().amax(1))[:, None]
    got = got.to(F64)
    delta = scale[:, None] * (p * E + 2.0 ** -23)
    report(name + " dlogits tight (elementwise)", ((got - bf(g)).abs() - 2 * U * g.abs() - 1.01 * delta).clamp_min(0).amax(1),
           torch.full((got.shape[0],), 1e-37, device=got.device, dtype=F64))
    bound = U * g.norm(dim=1) + scale * (E.squeeze(1) * p.norm(dim=1) + 2.0 ** -23) + 1e-37
    report(name + " dlogits loose (per row)", (got - g).norm(dim=1), bound)


@pytest.mark.parametrize("V,ldl", CE_SHAPES)
def test_cross_entropy_fwd_bwd_vs_fp64(ops, V, ldl):
    n, lg, tgt, buf = ce_case(V, ldl, seed=V)
    sentinel = buf[n:].clone()
    loss_sum = torch.full((1,), 3.25, device="cuda", dtype=F32)        # accumulates onto its previous value
    scale = torch.full((n,), 1.0 / n, device="cuda", dtype=F64)
    ops.cross_entropy_fwd_bwd(buf, tgt.to(torch.int32), loss_sum, n, V, 1.0 / n)
    torch.cuda.synchronize()
    lse, loss, p, g = ce_ref(lg, tgt, scale)
    assert (loss[8:] < 1e-4).all()                                     # the peaked rows do reach loss ~ 0
    # sum of the per-row bounds, plus the rounding of the running f32 atomic sum
    bound = lse_err(lse, lg.abs().amax(1)).sum() + 2.0 ** -23 * (loss.sum() + 3.25) * (n + 1)
    report(f"V={V} loss_sum", (loss_sum.double() - 3.25 - loss.sum()).abs(), bound)
    check_dlogits(f"V={V}", buf[:n, :V], lg, tgt, scale, lse, p, g)
    assert (buf[:n, V:] == 0).all(), "slack columns [V, ldl) must come back as exactly 0"
    assert torch.equal(buf[n:], sentinel), "rows past n must be left untouched"


@pytest.mark.parametrize("V,ldl", CE_SHAPES)
def test_cross_entropy_rows_vs_fp64(ops, V, ldl):
    n, lg, tgt, buf = ce_case(V, ldl, seed=V + 1)
    sentinel = buf[n:].clone()
    row_scale = torch.tensor([0.5, 0.0, 1.0, 1 / 3, 0.25, 0.0, 2.0, 1 / 7, 1.0, 0.0, 0.125, 1 / 12] + [9.0] * 4, device="cuda")
    row_loss = torch.full((16,), 7.5, device="cuda", dtype=F32)
    ops.cross_entropy_rows(buf, tgt.to(torch.int32), row_scale, row_loss, n, V)
    torch.cuda.synchronize()
    scale = row_scale[:n].double()
    lse, loss, p, g = ce_ref(lg, tgt, scale)
    report(f"V={V} row_loss (per row)", (row_loss[:n].double() - loss).abs(), lse_err(lse, lg.abs().amax(1)))
    assert (row_loss[n:] == 7.5).all(), "row_loss past n must be left untouched"
    zero = scale == 0
    assert (buf[:n][zero] == 0).all(), "a row with row_scale 0 must have exactly zero dlogits"
    keep = ~zero
    check_dlogits(f"V={V} rows", buf[:n, :V][keep], lg[keep], tgt[keep], scale[keep], lse[keep], p[keep], g[keep])
    assert (buf[:n, V:] == 0).all(), "slack columns [V, ldl) must come back as exactly 0"
    assert torch.equal(buf[n:], sentinel), "rows past n must be left untouched"


# ================================================================================================ B. loss head at Qwen3-4B width
def build_head_model(vocab):
    from vggt_qwen3_amd.qwen3 import Qwen3Config, Qwen3ForCausalLM
    m = Qwen3ForCausalLM(Qwen3Config(num_hidden_layers=1, vocab_size=VOCAB_QWEN), device="cuda", seed=11, init_on_device=True)
    g = torch.Generator(device="cuda").manual_seed(12)
    with torch.no_grad():      # norm weight ~ 3.5: logits of std ~ 3.5 (E has std 0.02 over 2560 columns)
        m._w["norm"].copy_((3.5 + 0.5 * torch.randn(m._w["norm"].shape, generator=g, device="cuda")).to(BF16))
    if vocab != VOCAB_QWEN:
        m.resize_token_embeddings(vocab)
        H = m.config.hidden_size
        o = m.table["embed"][0]
        pad = slice(o + vocab * H, o + m.vocab_p * H)
        assert m.vocab_p == 151680 and (m.flat_w[pad] == 0).all() and (m.flat_g[pad] == 0).all(), "pad rows left by shrinking"
    return m


@pytest.fixture(scope="module")
def head_models():
    cache = {}

    def get(vocab):
        if vocab not in cache:
            cache[vocab] = build_head_model(vocab)
        return cache[vocab]
    yield get
    cache.clear()


@pytest.fixture(scope="module")
def head_model(head_models):
    return head_models(VOCAB_VLM)


def collator_labels(B, L, n, vocab, seed, empty=2):
    """Labels laid out as the collator lays them out: -100 prompts, answer runs with a -100 hole, a run that ends at the last position
    (its last row has no target), a label at position 0 (never a target), and sample `empty` without any label. Returns labels [B, L]
    and the labelled rows (flat row t carries labels[t + 1]) with their targets, computed here independently of label_rows."""
    g = torch.Generator().manual_seed(seed)
    labels = torch.full((B, L), -100, dtype=torch.long)
    owners = [s for s in range(B) if s != empty]
    counts = [n // len(owners) + (1 if i < n % len(owners) else 0) for i in range(len(owners))]
    rows = torch.zeros(B, L, dtype=torch.bool)
    for s, c in zip(owners, counts):
        if c == 0:
            continue
        a = c // 2
        start = 7 + 3 * s
        rows[s, start:start + a] = True                         # first part of the answer
        if s == owners[0]:
            rows[s, L - 1 - (c - a):L - 1] = True               # the rest ends at the last position
        else:
            rows[s, start + a + 3:start + c + 3] = True         # a -100 hole of 3, then the rest
    t = rows.nonzero()
    labels[t[:, 0], t[:, 1] + 1] = torch.randint(0, vocab, (t.shape[0],), generator=g)
    labels[owners[-1], 0] = 5                                   # position 0: never a target
    idx = rows.reshape(-1).nonzero().squeeze(1)
    assert idx.numel() == n
    tgt = labels[:, 1:].reshape(B, L - 1)
    tgt = torch.cat([tgt, torch.full((B, 1), -100)], 1).reshape(-1)[idx]
    return labels, idx, tgt


def head_ref64(model, hs, hn_k, dlog_k, dE_k, tgt, scale, gscale):
    """fp64 loss head from the gathered bf16 rows hs [n, H], in CHUNK-column vocabulary chunks.
    Tight stage inputs: the kernel's hn_k and dlog_k (bf16). Loose: the unrounded chain from hs. Returns per-row / per-block errors
    and bounds, plus the fp64 d_hn of both chains (for the norm backward)."""
    c = model.config
    n, H = hs.shape
    V, eps = model.vocab, c.rms_norm_eps
    E = model._w["embed"]
    w = model._w["norm"].to(F64)
    x = hs.to(F64)
    rstd = torch.rsqrt(x.pow(2).mean(1, keepdim=True) + eps)
    hn_l = w * x * rstd
    hn_t = bf(w * bf(x * rstd))
    hn_kd = hn_k.to(F64)
    ar = torch.arange(n, device=hs.device)
    # pass 1: log-sum-exp of both chains, max |logit|, and the per-row rounding sensitivity s = max_j ||hn (.) E_j||
    m_l = torch.full((n,), -math.inf, device=hs.device, dtype=F64)
    m_t, s_l, s_t, lmax, sens = m_l.clone(), torch.zeros_like(m_l), torch.zeros_like(m_l), torch.zeros_like(m_l), torch.zeros_like(m_l)
    lt_l, lt_t = torch.zeros_like(m_l), torch.zeros_like(m_l)
    for v0 in range(0, V, CHUNK):
        v1 = min(V, v0 + CHUNK)
        Ec = E[v0:v1].to(F64)
        for lg, m, s in ((hn_l @ Ec.T, m_l, s_l), (bf(hn_kd @ Ec.T), m_t, s_t)):
            mn = torch.maximum(m, lg.amax(1))
            s.mul_(torch.exp(m - mn)).add_(torch.exp(lg - mn[:, None]).sum(1))
            m.copy_(mn)
            if s is s_l:
                lmax = torch.maximum(lmax, lg.abs().amax(1))
                sel = (tgt >= v0) & (tgt < v1)
                lt_l[sel] = lg[ar[sel], tgt[sel] - v0]
            else:
                lt_t[sel] = lg[ar[sel], tgt[sel] - v0]
        sens = torch.maximum(sens, (hn_l.pow(2) @ Ec.pow(2).T).sqrt().amax(1))
    lse_l, lse_t = m_l + s_l.log(), m_t + s_t.log()
    E_row = lse_err(lse_l, lmax)
    # |delta l_j| of the kernel's logits against the unrounded ones: hn carries two bf16 roundings (|eps| <= 2U, uniform: std
    # 2U / sqrt(3)) that reach l_j as a random-sign sum of std <= 2U / sqrt(3) ||hn (.) E_j||, taken at 6 sigma; then the logit's own
    # rounding U |l_j|.
    dl = 6 * 2 * U / math.sqrt(3) * sens + U * lmax
    # pass 2: dlogits, d_hn, dE (per 64-row block)
    acc = dict(et=torch.zeros_like(m_l), el=torch.zeros_like(m_l), g2=torch.zeros_like(m_l), gt2=torch.zeros_like(m_l),
               p2=torch.zeros_like(m_l), p2t=torch.zeros_like(m_l), pl=torch.zeros_like(m_l))
    d_hn_l = torch.zeros(n, H, device=hs.device, dtype=F64)
    d_hn_t = torch.zeros_like(d_hn_l)
    blk = {k: [] for k in ("et", "rt", "el", "rl")}
    for v0 in range(0, V, CHUNK):
        v1 = min(V, v0 + CHUNK)
        Ec = E[v0:v1].to(F64)
        lg_l, lg_t = hn_l @ Ec.T, bf(hn_kd @ Ec.T)
        p_l, p_t = torch.exp(lg_l - lse_l[:, None]), torch.exp(lg_t - lse_t[:, None])
        oh = torch.zeros_like(p_l)
        sel = (tgt >= v0) & (tgt < v1)
        oh[ar[sel], tgt[sel] - v0] = 1
        g_l, g_t = (p_l - oh) * scale[:, None], (p_t - oh) * scale[:, None]
        dk = dlog_k[:, v0:v1].to(F64)
        acc["et"] += (dk - bf(g_t)).pow(2).sum(1)
        acc["el"] += (dk - g_l).pow(2).sum(1)
        acc["g2"] += g_l.pow(2).sum(1)
        acc["gt2"] += g_t.pow(2).sum(1)
        acc["p2"] += p_l.pow(2).sum(1)
        acc["p2t"] += p_t.pow(2).sum(1)
        acc["pl"] = torch.maximum(acc["pl"], (p_t * lg_t.abs()).amax(1))
        d_hn_l += g_l @ Ec
        d_hn_t += dk @ Ec
        dE_t = gscale * dk.T @ hn_kd
        dE_l = gscale * g_l.T @ hn_l
        got = dE_k[v0:v1].to(F64)
        nb = (v1 - v0 + 63) // 64
        pad = nb * 64 - (v1 - v0)
        for key, ref in (("t", bf(dE_t)), ("l", dE_l)):
            e = torch.nn.functional.pad(got - ref, (0, 0, 0, pad)).view(nb, 64 * H).norm(dim=1)
            r = torch.nn.functional.pad(ref, (0, 0, 0, pad)).view(nb, 64 * H).norm(dim=1)
            blk["e" + key].append(e)
            blk["r" + key].append(r)
    gn, gnt = acc["g2"].sqrt(), acc["gt2"].sqrt()
    # tight dlogits: output rounding U ||g||; the f32 error of p (E ||p||, 2^-23 at the target); up to two logits whose bf16 rounding
    # flipped against fp64 (one ulp = 2U |l_j| moves p_j and, through the sum, every p: 2 * 2 * 2U * max_j p_j |l_j|)
    b_t = U * gnt + scale * (E_row * acc["p2t"].sqrt() + 2.0 ** -23 + 8 * U * acc["pl"])
    # loose dlogits: delta p_j = p_j (delta l_j - sum_k p_k delta l_k), so ||delta p|| <= 2 ||p|| max |delta l|, on top of the tight terms
    b_l = U * gn + scale * (E_row * acc["p2"].sqrt() + 2.0 ** -23 + 2 * acc["p2"].sqrt() * dl)
    out = dict(rstd=rstd, xh=x * rstd, hn_t=hn_t, hn_l=hn_l, lse=lse_l, lmax=lmax, E_row=E_row, dl=dl,
               loss_l=lse_l - lt_l, loss_t=lse_t - lt_t, pl=acc["pl"], dlog_t=(acc["et"].sqrt(), b_t),
               dlog_l=(acc["el"].sqrt(), b_l), rel_l=b_l / gn,
               d_hn_l=gscale * d_hn_l, d_hn_t=gscale * d_hn_t)
    out.update({k: torch.cat(v) for k, v in blk.items()})
    return out


def rms_bwd64(d_hn, xh, w, rstd):
    """fp64 RMSNorm backward: dx = rstd (d w - xh mean(d w xh)), dw = sum_rows d xh."""
    dw_ = d_hn * w
    return rstd * (dw_ - xh * (dw_ * xh).mean(1, keepdim=True)), (d_hn * xh).sum(0)


HEAD_CASES = [  # (vocab, n labelled rows, expected K slices of the lm_head input gradient, atomic split forced)
    (VOCAB_VLM, 1, 10, False), (VOCAB_VLM, 61, 10, False), (VOCAB_VLM, 250, 6, False), (VOCAB_VLM, 1203, 2, False),
    (VOCAB_QWEN, 250, 2, False), (VOCAB_VLM, 250, 1, True),
]


@pytest.mark.parametrize("groups", [None, [2, 1, 3]], ids=["one-loss", "groups"])
@pytest.mark.parametrize("vocab,n,S,atomic", HEAD_CASES, ids=[f"V{v}-n{n}-S{s}" for v, n, s, _ in HEAD_CASES])
def test_loss_head_vs_fp64(head_models, monkeypatch, vocab, n, S, atomic, groups):
    from vggt_qwen3_amd.qwen3 import Qwen3ForCausalLM
    if atomic:
        monkeypatch.setenv("VQ3_LMHEAD_DGRAD_ATOMIC", "1")
    model = head_models(vocab)
    H, Vp = model.config.hidden_size, model.vocab_p
    n8 = (n + 7) // 8 * 8
    assert Qwen3ForCausalLM._lm_dgrad_slices(Vp, ((n8 + 127) // 128) * ((H + 127) // 128)) == S
    B, L = 6, 320
    labels, idx, tgt = collator_labels(B, L, n, vocab, seed=n)
    gh = torch.Generator(device="cuda").manual_seed(n + 1)
    h_last = (torch.randn(B * L, H, generator=gh, device="cuda") *
              (0.5 + torch.rand(B * L, 1, generator=gh, device="cuda"))).to(BF16)
    idx, tgt = idx.cuda(), tgt.cuda()
    # a few targets at column 0, at V - 1 and at the row's (fp64) maximum
    tgt[0] = 0
    if n > 2:
        tgt[1] = vocab - 1
        x = h_last[idx[2]].double()
        hn = bf(model._w["norm"].double() * bf(x * torch.rsqrt(x.pow(2).mean() + model.config.rms_norm_eps)))
        tgt[2] = torch.cat([model._w["embed"][v0:v0 + CHUNK].double() @ hn for v0 in range(0, vocab, CHUNK)]).argmax()
    labels.view(-1)[(idx + 1).cpu()] = tgt.cpu()
    gscale = 0.75
    loss, ctx = model.loss_head(h_last, labels.cuda(), save=True, L=L, groups=groups)
    assert ctx["n"] == n and torch.equal(ctx["idx"].long(), idx)
    dlog_k = ctx["dlogits"][:n].clone()
    dh = model.backward_loss_head(ctx, B * L, gscale, accumulate=False)
    dE_full = model.flat_g[model.table["embed"][0]: model.table["embed"][0] + Vp * H].view(Vp, H)
    dE_k, dn_k, dh_k = dE_full.clone(), model._g["norm"].clone(), dh.clone()
    torch.cuda.synchronize()
    # the gradient parts of one run: finite, zero where nothing can reach them
    for name, t in (("dh", dh_k), ("dE", dE_k), ("d(norm)", dn_k)):
        assert torch.isfinite(t.float()).all(), f"non-finite values in {name}"
    lab_rows = torch.zeros(B * L, dtype=torch.bool, device="cuda")
    lab_rows[idx] = True
    assert (dh_k[~lab_rows] == 0).all(), "rows without a label must have exactly zero dh"
    assert (dE_k[vocab:] == 0).all(), "rows vocab..Vp of the embedding gradient must stay exactly 0"
    assert (ctx["dlogits"][:, vocab:] == 0).all() and (ctx["dlogits"][n:] == 0).all()
    # row scales: each group's rows are normalised by that group's number of labelled rows
    if groups is None:
        scale = torch.full((n,), 1.0 / n, device="cuda", dtype=F64)
        gid = torch.zeros(n, dtype=torch.long, device="cuda")
    else:
        gid = torch.repeat_interleave(torch.arange(len(groups)), torch.tensor(groups)).cuda()[idx // L]   # sample -> its group
        cnt = torch.bincount(gid, minlength=len(groups)).double()
        scale = 1.0 / cnt[gid]
    ref = head_ref64(model, h_last[idx], ctx["hn"][:n], dlog_k, dE_k, tgt.long(), scale, gscale)
    tag = f"V={vocab} n={n} S={S} groups={groups}"
    # forward: hn within two ulps of the rounded restatement - the kernel rounds x * rstd from f32 (rstd's own error, double rounding),
    # so the inner bf16 value may be the fp64 one's neighbour, which w (~3.5) and the outer rounding make at most two ulps of hn;
    # logits of std >= 3
    report(tag + " hn tight (elementwise)", ((ctx["hn"][:n].double() - ref["hn_t"]).abs() - 4 * U * ref["hn_t"].abs()).clamp_min(0)
           .amax(1), torch.full((n,), 1e-30, device="cuda", dtype=F64))
    if n > 100:
        assert ref["lmax"].mean() > 3 * 3.0, "logits must spread (std >= 3)"
    # loss: no rounding point of its own; per row |delta| <= |delta l_t| + sum_j p_j |delta l_j| + E <= 2 max |delta l| + E
    row_b = 2 * ref["dl"] + ref["E_row"]
    if groups is None:
        report(tag + " loss loose", (loss.double() - ref["loss_l"].mean()).abs().reshape(1), row_b.mean().reshape(1))
    else:
        cnt = torch.bincount(gid, minlength=len(groups))
        for k in range(len(groups)):
            if cnt[k] == 0:
                assert torch.isnan(loss[k]), "a group without a label has a NaN loss"
            else:
                sel = gid == k
                report(tag + f" loss[{k}] loose", (loss[k].double() - ref["loss_l"][sel].mean()).abs().reshape(1),
                       row_b[sel].mean().reshape(1))
    # tight loss: fp64 cross entropy of bf16(hn_k E^T); per row E, plus up to two flipped logits (2U |l_j| each, weighted by p_j)
    # and one flip of the target's own logit in the whole group (2U max |l|)
    tb = lambda sel: (ref["E_row"][sel] + 8 * U * ref["pl"][sel]).mean() + 2 * U * ref["lmax"][sel].max() / int(sel.sum())
    if groups is None:
        sel = torch.ones(n, dtype=torch.bool, device="cuda")
        report(tag + " loss tight", (loss.double() - ref["loss_t"].mean()).abs().reshape(1), tb(sel).reshape(1))
    else:
        for k in range(len(groups)):
            sel = gid == k
            if sel.any():
                report(tag + f" loss[{k}] tight", (loss[k].double() - ref["loss_t"][sel].mean()).abs().reshape(1), tb(sel).reshape(1))
    report(tag + " dlogits tight (per row)", *ref["dlog_t"])
    report(tag + " dlogits loose (per row)", *ref["dlog_l"])
    # dE per 64-row block. Tight: from the kernel's own dlogits and hn: the output rounding U, the f32 sum over n8 rows (< 1e-3
    # relative at n = 1203 with random signs). Loose: hn carries 2U, the output U, and the dlogits of the block: a block that holds a
    # target carries the rows' relative error rel_l, any other block only p_j, whose relative error is |delta l_j - sum p delta l|
    # <= 2 max |delta l| (dl) - both taken at their largest over the rows. Floor: 1e-3 of the largest block norm.
    nbv = (vocab + 63) // 64
    for key, bound in (("t", U + 1e-3), ("l", 3 * U + 1e-3 + max(ref["rel_l"].max().item(), 2 * ref["dl"].max().item()))):
        e, r = ref["e" + key][:nbv], ref["r" + key][:nbv]
        report(tag + f" dE {'tight' if key == 't' else 'loose'} (per 64-row block)", e, bound * r.clamp_min(1e-3 * r.max()))
    # dh per row and d(norm.weight). Tight: the kernel's dlogits through bf16(d_hn) (the f32 K-slice sums of 151 680 terms: < 1e-4
    # relative) and the fp64 norm backward; the output rounding U and a possible one-ulp flip of d_hn: 2U + 1e-4 (d(norm): the f32
    # sum over the rows adds 1e-3). Loose: the fp64 chain throughout; the row's dlogits error rel_l reaches d_hn at most twice over
    # (E's rows mix it), then the roundings of d_hn and of dh: 2 rel_l + 3U.
    w, xh, rstd = model._w["norm"].double(), ref["xh"], ref["rstd"]
    dh_t, dw_t = rms_bwd64(bf(ref["d_hn_t"]), xh, w, rstd)
    dh_l, dw_l = rms_bwd64(ref["d_hn_l"], xh, w, rstd)
    got = dh_k[idx].double()
    report(tag + " dh tight (per row)", (got - dh_t).norm(dim=1), (2 * U + 1e-4) * dh_t.norm(dim=1))
    report(tag + " dh loose (per row)", (got - dh_l).norm(dim=1), (2 * ref["rel_l"] + 3 * U) * dh_l.norm(dim=1))
    report(tag + " d(norm) tight", (dn_k.double() - dw_t).norm().reshape(1), ((2 * U + 1e-3) * dw_t.norm()).reshape(1))
    report(tag + " d(norm) loose", (dn_k.double() - dw_l).norm().reshape(1),
           ((2 * ref["rel_l"].max() + 3 * U) * dw_l.norm()).reshape(1))
    if S > 1:   # the sliced split is a fixed sequence of f32 sums: the same bits run after run
        _, ctx2 = model.loss_head(h_last, labels.cuda(), save=True, L=L, groups=groups)
        dh2 = model.backward_loss_head(ctx2, B * L, gscale, accumulate=False)
        assert torch.equal(dh2, dh_k) and torch.equal(dE_full, dE_k) and torch.equal(model._g["norm"], dn_k), \
            "the sliced lm_head backward must be bit-repeatable"
    if n == 250 and groups is None and not atomic:
        # accumulate=True adds to what is there: bf16(old + new) from the kernel's own dlogits and hn (tight per block: U + f32 sum)
        h2 = torch.roll(h_last, 1, 0)
        _, ctx2 = model.loss_head(h2, labels.cuda(), save=True, L=L)
        model.backward_loss_head(ctx2, B * L, gscale, accumulate=True)
        add = gscale * ctx2["dlogits"][:n, :vocab].double().T @ ctx2["hn"][:n].double()
        want = bf(dE_k[:vocab].double() + add)
        nb = vocab // 64
        e = (dE_full[:nb * 64].double() - want[:nb * 64]).view(nb, -1).norm(dim=1)
        r = want[:nb * 64].view(nb, -1).norm(dim=1)
        report(tag + " dE accumulate tight (per 64-row block)", e, (U + 1e-3) * r)
        assert (dE_full[vocab:] == 0).all()


# ================================================================================================ C. embedding / splice backward
def embed_case(H, seed, V=4096, B=4, L=640, S=96):
    """ids with runs of 1, 15, 16, 17, 64, 65 rows and the padding id's run of >= 1000 rows, scattered over the batch; a spliced span
    (srcmap >= 0) per sample that takes 3 rows of every run of 15 and more and every occurrence of one id (`spliced_only`)."""
    g = torch.Generator().manual_seed(seed)
    T = B * L
    srcmap = torch.full((B, L), -1, dtype=torch.int32)
    for b in range(B):
        s0 = 20 + 37 * b
        srcmap[b, s0:s0 + S] = torch.arange(S, dtype=torch.int32)
    flat_sp = (srcmap.reshape(-1) >= 0).nonzero().squeeze(1)
    flat_sp = flat_sp[torch.randperm(flat_sp.numel(), generator=g)].tolist()
    flat_pl = (srcmap.reshape(-1) < 0).nonzero().squeeze(1)
    flat_pl = flat_pl[torch.randperm(flat_pl.numel(), generator=g)].tolist()
    ids = torch.randint(2300, V, (T,), generator=g)               # everything else: random ids, runs of 1-3
    spliced_only = 2222
    runs = {7: 1, 100: 15, 200: 16, 300: 17, 400: 64, 500: 65, 1: 1010}   # id -> run length (1: the padding id)
    for i, r in runs.items():
        k = 3 if r >= 15 else 0
        for _ in range(k):
            ids[flat_sp.pop()] = i
        for _ in range(r - k):
            ids[flat_pl.pop()] = i
    for _ in range(5):
        ids[flat_sp.pop()] = spliced_only
    return ids.view(B, L).cuda(), srcmap.cuda(), spliced_only


def embed_bwd_ref(ids, srcmap, dout, dtable0):
    """fp64 index_add of the non-spliced rows of dout onto the table."""
    H = dout.shape[-1]
    keep = (srcmap < 0).reshape(-1)
    ref = dtable0.to(F64).clone()
    ref.index_add_(0, ids.reshape(-1)[keep], dout.reshape(-1, H)[keep].to(F64))
    return ref


def check_table(tag, got, ref, touched):
    """Per table row. Tight: bf16(fp64 sum) - the output rounding of both is the same, so what is left is the f32 sum (runs of up to
    ~1100 rows: < 1e-4 relative with random signs) and a one-ulp flip now and then: 2U per element at most, U + 1e-4 per row. Loose:
    the unrounded sum: the output rounding U plus the f32 sum, 1.01 U + 1e-4. Floor: 1e-3 of the largest row norm."""
    got = got[touched].to(F64)
    ref = ref[touched]
    rn = ref.norm(dim=1).clamp_min(1e-3 * ref.norm(dim=1).max())
    report(tag + " tight (per row)", (got - bf(ref)).norm(dim=1), (U + 1e-4) * rn)
    report(tag + " loose (per row)", (got - ref).norm(dim=1), (1.01 * U + 1e-4) * rn)


@pytest.mark.parametrize("H", [2560, 1000])
def test_embed_splice_bwd_vs_fp64(ops, H):
    V, B, L, S = 4096, 4, 640, 96
    ids, srcmap, spliced_only = embed_case(H, seed=H)
    g = torch.Generator(device="cuda").manual_seed(H + 1)
    dout = torch.randn(B, L, H, generator=g, device="cuda").to(BF16)
    dtable = (0.1 * torch.randn(V, H, generator=g, device="cuda")).to(BF16)
    dtable0 = dtable.clone()
    dfeat = torch.zeros((B, S, H), device="cuda", dtype=F32)
    sorted_ids, order = torch.sort(ids.reshape(-1), stable=True)
    ops.embed_splice_bwd(sorted_ids, order, srcmap, dout, dtable, dfeat, B, L, H, S)
    torch.cuda.synchronize()
    ref = embed_bwd_ref(ids, srcmap, dout, dtable0)
    live = torch.zeros(V, dtype=torch.bool, device="cuda")
    live[ids.reshape(-1)[(srcmap < 0).reshape(-1)]] = True
    assert not live[spliced_only]
    # rows that receive nothing - ids never seen, and the id whose every occurrence is spliced - stay bit-identical (not re-rounded)
    assert torch.equal(dtable[~live], dtable0[~live])
    check_table(f"embed_bwd H={H}", dtable, ref, live)
    for i, r in ((7, 1), (100, 15), (200, 16), (300, 17), (400, 64), (500, 65), (1, 1010)):
        e = ((dtable[i].double() - ref[i]).norm() / ref[i].norm()).item()
        assert e < U + 1e-4, f"id {i} (run of {r}): rel err {e}"
    # dfeat: every (b, s) is fed by exactly one position: exact
    reff = torch.zeros_like(dfeat)
    for b in range(B):
        sel = srcmap[b] >= 0
        reff[b, srcmap[b, sel].long()] = dout[b, sel].float()
    assert torch.equal(dfeat, reff)


def test_tied_embedding_gradient_both_contributions(head_model, ops):
    """The tied table at Vp = 151 680 after both contributions, in the order _backward_text applies them: backward_loss_head
    (accumulate=False) writes the lm_head part, then the lookup backward adds the input-embedding part."""
    model = head_model
    H, Vp, vocab = model.config.hidden_size, model.vocab_p, model.vocab
    B, L, n = 6, 320, 61
    labels, idx, tgt = collator_labels(B, L, n, vocab, seed=3)
    g = torch.Generator(device="cuda").manual_seed(4)
    h_last = torch.randn(B * L, H, generator=g, device="cuda").to(BF16)
    loss, ctx = model.loss_head(h_last, labels.cuda(), save=True, L=L)
    model.backward_loss_head(ctx, B * L, 1.0, accumulate=False)
    dE_full = model.flat_g[model.table["embed"][0]: model.table["embed"][0] + Vp * H].view(Vp, H)
    head_part = dE_full.clone()
    ids = torch.randint(0, vocab, (B, L), generator=g, device="cuda")
    ids[:, 200:] = 151643                                          # the padding id's run: 720 rows
    ids[0, :3] = vocab - 1
    srcmap = torch.full((B, L), -1, dtype=torch.int32, device="cuda")
    srcmap[:, 10:74] = torch.arange(64, dtype=torch.int32, device="cuda")
    dout = (1e-2 * torch.randn(B, L, H, generator=g, device="cuda")).to(BF16)
    sorted_ids, order = torch.sort(ids.reshape(-1), stable=True)
    ops.embed_splice_bwd(sorted_ids, order, srcmap, dout, dE_full, None, B, L, H, 64)
    torch.cuda.synchronize()
    ref = embed_bwd_ref(ids, srcmap, dout, head_part[:vocab])
    touched = torch.zeros(vocab, dtype=torch.bool, device="cuda")
    touched[ids.reshape(-1)[(srcmap < 0).reshape(-1)]] = True
    assert touched[vocab - 1] and touched[151643]
    assert torch.equal(dE_full[:vocab][~touched], head_part[:vocab][~touched])
    assert (dE_full[vocab:] == 0).all(), "rows vocab..Vp of the tied gradient must stay exactly 0"
    check_table("tied dE (lm_head + lookup)", dE_full[:vocab], ref, touched)


# ================================================================================================ D. the live-rows path
def live_batch(z, L=320):
    """The tiny golden batch stretched to L = 320 (~85 % padding): samples 1 and 3 left-padded, the rest right-padded, and labels on
    masked positions - one whose row is masked and predicts a real token (left padding), and two past the end of a right-padded row."""
    import numpy as np
    ids0, mask0, lab0 = (torch.from_numpy(np.asarray(z[k])) for k in ("input_ids", "attention_mask", "labels"))
    B, L0 = ids0.shape
    ids = torch.full((B, L), 1, dtype=torch.long)
    mask = torch.zeros(B, L, dtype=torch.long)
    labels = torch.full((B, L), -100, dtype=torch.long)
    for b in range(B):
        m = int(mask0[b].sum())
        off = 40 + 9 * b if b in (1, 3) else 0                 # left padding
        ids[b, off:off + m], mask[b, off:off + m], labels[b, off:off + m] = ids0[b, :m], 1, lab0[b, :m]
    labels[1, 40 + 9] = 77                                      # first real token of a left-padded row: row 48 (masked) predicts it
    m0 = int(mask0[0].sum())
    labels[0, m0 + 2], labels[0, m0 + 5] = 81, 82               # past the end of a right-padded row (rows m0 + 1, m0 + 4 are masked)
    assert (mask == 0).float().mean() > 0.8
    return ids, mask, labels


def test_live_rows_dead_rows_have_zero_gradient_and_route_is_bit_identical(monkeypatch):
    import numpy as np
    from tests.golden_io import load, meta
    from tests.test_parity_gpu import _build_vlm
    z = load("vlm_tiny.npz")
    m = meta(z)
    ids, mask, labels = live_batch(z)
    images = torch.from_numpy(z["pixel_values"].astype(np.float32)).cuda()
    geom = {k: torch.from_numpy(z["geom:" + k]).cuda() for k in ("R", "t", "K", "depth_hist")}
    geom["mask"] = torch.from_numpy(z["geom_mask"]).cuda()
    res = {}
    for live_env in ("0", "1"):
        monkeypatch.setenv("VQ3_EMBED_BWD_LIVE", live_env)
        model = _build_vlm(z, m).train()
        model.train_projector = True
        tm = model.text_model
        st = model.forward_state(images, geom, ids.cuda(), mask.cuda(), labels.cuda(), need_grad=True)
        assert st["L"] == 320 and st["live"] is not None
        if live_env == "1":
            # d(inputs_embeds) straight from backward_hidden: exactly 0 on every row the VLM calls dead
            Bq, Lp = st["B"], st["saved"]["L"]
            dh = tm.backward_loss_head(st["head"], Bq * Lp, 1.0, accumulate=False)
            d_emb = tm.backward_hidden(st["saved"], dh, accumulate=False).view(Bq, Lp, -1)[:, :st["L"]]
            live = st["live"]
            assert (~live).float().mean() > 0.8
            assert (d_emb[~live] == 0).all(), "a row the live-rows path skips has a nonzero d(inputs_embeds)"
            for b, l in ((1, 48), (0, int(z["attention_mask"][0].sum()) + 1)):   # masked rows that carry a label are live and matter
                assert live[b, l] and mask[b, l] == 0 and d_emb[b, l].abs().max() > 0
            st = model.forward_state(images, geom, ids.cuda(), mask.cuda(), labels.cuda(), need_grad=True)
        d_geom = model._backward_text(st, 1.0, accumulate=False)
        torch.cuda.synchronize()
        pg = [p.grad.clone() if p.grad is not None else None for p in model.projector.parameters()]
        assert any(t is not None for t in pg)
        res[live_env] = (tm.flat_g.clone(), d_geom.clone(), pg)
    (g0, d0, p0), (g1, d1, p1) = res["0"], res["1"]
    assert torch.equal(g0, g1), "the live-rows path must leave a bit-identical flat_g"
    assert torch.equal(d0, d1)
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(p0, p1)), "projector gradients differ"
