"""Qwen3 attention at the lengths the model trains and infers at: the fused causal GQA kernels (qwen_flash.hip: forward, dQ, the
dK / dV kernel) up to their L = 8192 cap and the decode attention (decode.hip) up to its 12 288-row cache, against a plain fp64
restatement of the same operation. Errors are measured per 32-row block, so one wrong block cannot hide in a long tensor's norm."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
LOG2E = 1.4426950408889634
D = 128
SCALE = D ** -0.5
# per-block bounds (the short test's whole-tensor numbers, per block) and the absolute floor of a block's reference norm: a block
# whose fp64 norm is below BLOCK_FLOOR is held to bound * BLOCK_FLOOR in absolute terms. Unit-normal operands give block norms of
# 3e-2 and more everywhere (the last key block at L = 8192 is the smallest); only rows that one spiked key saturates come near 0.
O_TOL, DQ_TOL, DKV_TOL, LSE_TOL = 1e-2, 2e-2, 2e-2, 2e-2
BLOCK_FLOOR = 1e-3


@pytest.fixture(scope="module")
def ops():
    from vggt_qwen3_amd import _lib
    from vggt_qwen3_amd import ops as _ops
    _lib.load()
    return _ops


# ------------------------------------------------------------------------------------------------ fp64 reference
def attn_ref64(Q, K, V, dO, mask, scale=SCALE, O_in=None, bwd=True, chunk=1024):
    """Causal GQA attention in fp64 from the same bf16 operands. Q [B,Hq,L,D], K / V [B,Hkv,L,D], dO [B*L, Hq*D] token-major,
    mask uint8 [B,L] (1 = attended key). Returns O [B,Hq,L,D], LSE [B,Hq,L] (log2 domain of the scaled scores, +inf on rows with
    no attended key), and with bwd dQ [B,Hq,L,D], dK / dV [B,Hkv,L,D] from the explicit formulas P, dP = dO V^T,
    dS = P o (dP - delta), delta = rowsum(P o dP) - or rowsum(dO o O_in) when O_in (the bf16 O the backward is given) is passed.
    Rows with no attended key have P = 0. Query rows go in chunks: no L x L tensor, no autograd."""
    B, Hq, L, _ = Q.shape
    Hkv = K.shape[1]
    G = Hq // Hkv
    dev = Q.device
    O = torch.zeros(B, Hq, L, D, device=dev, dtype=F64)
    lse = torch.full((B, Hq, L), math.inf, device=dev, dtype=F64)
    dQ = torch.zeros_like(O) if bwd else None
    dK = torch.zeros(B, Hkv, L, D, device=dev, dtype=F64) if bwd else None
    dV = torch.zeros_like(dK) if bwd else None
    dOh = dO.view(B, L, Hq, D).permute(0, 2, 1, 3) if bwd else None
    Oin = O_in.view(B, L, Hq, D).permute(0, 2, 1, 3) if O_in is not None else None
    ar = torch.arange(L, device=dev)
    keyok = mask.bool()
    for b in range(B):
        for hk in range(Hkv):
            k, v = K[b, hk].double(), V[b, hk].double()
            for q0 in range(0, L, chunk):
                q1 = min(L, q0 + chunk)           # causal: keys past the chunk's last row never count
                vis = (ar[None, :q1] <= ar[q0:q1, None]) & keyok[b, None, :q1]
                rowok = vis.any(1, keepdim=True)
                kk, vv = k[:q1], v[:q1]
                for hq in range(hk * G, hk * G + G):
                    q = Q[b, hq, q0:q1].double()
                    s = (q @ kk.T * scale).masked_fill(~vis, -math.inf)
                    m = torch.where(rowok, s.amax(1, keepdim=True), torch.zeros((), device=dev, dtype=F64))
                    e = torch.exp(s - m)
                    l = e.sum(1, keepdim=True)
                    p = e / torch.where(rowok, l, torch.ones((), device=dev, dtype=F64))
                    O[b, hq, q0:q1] = p @ vv
                    lse[b, hq, q0:q1] = torch.where(rowok, (m + l.log()) * LOG2E, math.inf).squeeze(1)
                    if not bwd:
                        continue
                    do = dOh[b, hq, q0:q1].double()
                    dp = do @ vv.T
                    delta = (p * dp).sum(1, keepdim=True) if Oin is None else (do * Oin[b, hq, q0:q1].double()).sum(1, keepdim=True)
                    ds = p * (dp - delta)
                    dQ[b, hq, q0:q1] = ds @ kk * scale
                    dK[b, hk, :q1] += ds.T @ q * scale
                    dV[b, hk, :q1] += p.T @ do
    return O, lse, dQ, dK, dV


def _block_err(got, ref, rows_ok=None):
    """Per 32-row block of the second-to-last axis: ||got - ref|| / max(||ref||, BLOCK_FLOOR). rows_ok [..., L] leaves rows out."""
    got, ref = got.double(), ref.double()
    if rows_ok is not None:
        keep = rows_ok[..., None].to(F64)
        got, ref = got * keep, ref * keep
    L = got.shape[-2]
    pad = (-L) % 32
    diff = torch.nn.functional.pad(got - ref, (0, 0, 0, pad)).unflatten(-2, (-1, 32))
    refb = torch.nn.functional.pad(ref, (0, 0, 0, pad)).unflatten(-2, (-1, 32))
    dn = diff.pow(2).sum((-1, -2)).sqrt()
    rn = refb.pow(2).sum((-1, -2)).sqrt()
    return dn / rn.clamp_min(BLOCK_FLOOR)


def _assert_blocks(name, got, ref, bound, rows_ok=None):
    err = _block_err(got, ref, rows_ok)
    worst = int(err.flatten().argmax())
    where = [int(i) for i in torch.unravel_index(torch.tensor(worst), tuple(err.shape))]
    assert err.max().item() <= bound, f"{name}: block {where} (last index = 32-row block) error {err.max().item():.3e} > {bound}"


def check_attention(mask, Hq, O, lse, ref, dQ=None, dK=None, dV=None):
    """The per-block statement shared by every Qwen flash test. O token-major [B*L, Hq*D] (kernel), lse [B,Hq,L]; ref from
    attn_ref64. Dead query rows (no attended key at or before them): O = dQ = 0 and LSE = +inf exactly; masked key rows: dK = dV = 0
    exactly; everything finite; the rest within O_TOL / DQ_TOL / DKV_TOL per (b, head, 32-row block) and LSE_TOL absolute."""
    B, L = mask.shape
    rO, rlse, rdQ, rdK, rdV = ref
    Oh = O.view(B, L, Hq, D).permute(0, 2, 1, 3)
    keyok = mask.bool()
    alive = (keyok.int().cumsum(1) > 0)[:, None, :].expand(B, Hq, L)          # some attended key at or before the row
    assert torch.isfinite(Oh.float()).all(), "O not finite"
    assert torch.isfinite(lse[alive]).all() and (lse[~alive] == math.inf).all(), "LSE: dead rows must be +inf, live rows finite"
    assert (lse[alive].double() - rlse[alive]).abs().max().item() <= LSE_TOL, "LSE"
    assert (Oh[~alive] == 0).all(), "O of a dead query row must be exactly 0"
    _assert_blocks("O", Oh, rO, O_TOL, alive)
    if dQ is None:
        return
    for name, t in (("dQ", dQ), ("dK", dK), ("dV", dV)):
        assert torch.isfinite(t.float()).all(), f"{name} not finite"
    assert (dQ[~alive] == 0).all(), "dQ of a dead query row must be exactly 0"
    Hkv = dK.shape[1]
    dead_key = ~keyok[:, None, :].expand(B, Hkv, L)
    assert (dK[dead_key] == 0).all() and (dV[dead_key] == 0).all(), "dK / dV of a masked key must be exactly 0"
    _assert_blocks("dQ", dQ, rdQ, DQ_TOL)
    _assert_blocks("dK", dK, rdK, DKV_TOL)
    _assert_blocks("dV", dV, rdV, DKV_TOL)


def _operands(B, Hkv, G, L, seed):
    g = torch.Generator().manual_seed(seed)
    Hq = G * Hkv
    Q = torch.randn(B, Hq, L, D, generator=g)
    K = torch.randn(B, Hkv, L, D, generator=g)
    V = torch.randn(B, Hkv, L, D, generator=g)
    dO = torch.randn(B * L, Hq * D, generator=g)
    return Q, K, V, dO


def _cuda(*ts):
    return [t.to(BF16).cuda() for t in ts]


def _mask(B, L, kind):
    m = torch.ones(B, L, dtype=torch.uint8)
    if kind == "stage2":              # row 1 attends 1000 keys: 96 trailing key tiles of 128 drop out
        m[1, 1000:] = 0
    elif kind == "left":              # row 1 starts at 700: query blocks 0-20 dead, block 21 partly
        m[1, :700] = 0
    elif kind == "holes":
        m[0, :41] = 0                 # rows 0-40 dead; row 41's only attended key is itself
        m[0, 64:192] = 0              # four whole key tiles in the middle of every later row
        m[0, 200::37] = 0             # scattered single keys
        m[0, L - 3] = 0
    elif kind == "stage1":            # row 1 attends 37 keys
        m[1, 37:] = 0
    return m.cuda()


def run_case(ops, B, Hkv, G, L, kind, seed, bwd=True, kv_parts=1):
    Q, K, V, dO = _cuda(*_operands(B, Hkv, G, L, seed))
    mask = _mask(B, L, kind)
    Hq = G * Hkv
    O, lse = ops.qwen_flash_fwd(Q, K, V, mask, B, L, Hq, Hkv, D, SCALE)
    grads = ops.qwen_flash_bwd(Q, K, V, mask, O, dO, lse, B, L, Hq, Hkv, D, SCALE, kv_parts=kv_parts) if bwd else (None,) * 3
    if bwd and kv_parts > 1:                              # partial dK / dV slabs: their sum is the gradient
        grads = (grads[0], grads[1].float().sum(0), grads[2].float().sum(0))
    ref = attn_ref64(Q, K, V, dO, mask, bwd=bwd)
    check_attention(mask, Hq, O, lse, ref, *grads)


# ------------------------------------------------------------------------------------------------ prefill / training kernels
@pytest.mark.parametrize("B,Hkv,G,L,kind", [(1, 1, 4, 8192, "dense"), (2, 2, 4, 4096, "stage2"), (2, 1, 4, 2056, "left"),
                                            (1, 2, 2, 1032, "holes"), (2, 1, 4, 512, "stage1"), (1, 8, 4, 2048, "dense")],
                         ids=["cap-8192", "stage2-4096", "left-2056", "holes-1032", "stage1-512", "heads-32x8-2048"])
def test_qwen_flash_long_vs_fp64(ops, B, Hkv, G, L, kind):
    """Forward, dQ and dK / dV at the cap, Stage-2 right padding (trailing key tiles dropped), left padding (whole dead query
    blocks: O = dQ = 0, LSE = +inf), holes in the middle of rows, Stage-1 length and Qwen3-4B's 32 / 8 heads."""
    run_case(ops, B, Hkv, G, L, kind, seed=L + B)


def _spiked_operands(L=4096):
    """B = 1, Hkv = 1, G = 4. K[j] = f Q[h, q]: the score of (q, j) is ~ f |Q|^2 / sqrt(D) ~ 11 f in natural units."""
    Q, K, V, dO = _operands(1, 1, 4, L, seed=11)
    mask = torch.ones(1, L, dtype=torch.uint8)
    mask[0, L - 6:] = 0                                  # the last tile is partly attended
    mask[0, 3000] = 0
    Q[0, 0, 40:3000:13] = Q[0, 0, 40]                    # ~230 rows of head 0 share one query ...
    spikes = [(5, 0, 40, 6.0),                           # ... and key 5 (tile 0) is their attention sink
              (2500, 1, 3100, 8.5),                      # tile 78: e^(score) is past fp32 unless the running max is applied there
              (L - 9, 2, L - 2, 5.0),                    # the last, partly attended tile
              (1777, 3, 1777, 5.0),                      # the diagonal
              (3000, 2, 3500, 9.0),                      # a masked key: no effect
              (3600, 1, 3590, 9.0)]                      # above the diagonal: no effect on row 3590
    for j, h, q, f in spikes:
        K[0, 0, j] = f * Q[0, h, q]
    return Q, K, V, dO, mask, spikes


def test_qwen_flash_spiked_scores(ops):
    """Rare data-dependent branches of the online softmax: a late tile whose score exceeds everything before it by far more than
    fp32's exponent range (the rescale alpha of earlier tiles underflows to 0), a sink in tile 0, spikes in the last partial tile and
    on the diagonal, and spikes that the masks must hide. Forward and backward within the per-block bounds."""
    Q, K, V, dO, mask, spikes = _spiked_operands()
    L = Q.shape[2]
    s_late = float((Q[0, 1, 3100].to(BF16).double() @ K[0, 0, 2500].to(BF16).double()) * SCALE)
    assert s_late > 90.0, s_late                          # e^90 > fp32 max: the construction does what it claims
    Q, K, V, dO = _cuda(Q, K, V, dO)
    mask = mask.cuda()
    O, lse = ops.qwen_flash_fwd(Q, K, V, mask, 1, L, 4, 1, D, SCALE)
    dQ, dK, dV = ops.qwen_flash_bwd(Q, K, V, mask, O, dO, lse, 1, L, 4, 1, D, SCALE)
    # The backward is given the bf16 O and forms delta = rowsum(dO o O) from it (FlashAttention-2's form). Where one key holds all
    # but 1e-4 .. 1e-2 of a row's weight - the cross-talk of the x8.5 / x9 keys with ~3 % of the other rows - the exact dP_j - delta
    # is ~(1 - P_j) * 11, below the ~2^-9 * |dO| |O| ~ 1e-2 that O's own bf16 rounding puts into delta; so the reference takes delta
    # from the same bf16 O. The forward, which produces that O, is held to the exact reference above it.
    ref = attn_ref64(Q, K, V, dO, mask, O_in=O)
    check_attention(mask, 4, O, lse, ref, dQ, dK, dV)
    Oh = O.view(L, 4, D)
    # the sink and the diagonal spike saturate their rows: O is the spiked key's value row
    assert (Oh[40:3000:13, 0].float() - V[0, 0, 5].float()).abs().max().item() < 2e-2
    assert (Oh[1777, 3].float() - V[0, 0, 1777].float()).abs().max().item() < 2e-2
    assert (Oh[3100, 1].float() - V[0, 0, 2500].float()).abs().max().item() < 2e-2


@pytest.mark.parametrize("bad", ["L", "G", "kv_parts"])
def test_qwen_flash_rejects_out_of_range(ops, bad):
    from vggt_qwen3_amd._lib import Vq3Error
    B, Hkv, G, L = 1, 1, 4, 64
    if bad == "L":
        L = 8193
    if bad == "G":
        G = 8
    Hq = G * Hkv
    Q, K, V, dO = _cuda(*_operands(B, Hkv, G, L, seed=1))
    mask = torch.ones(B, L, dtype=torch.uint8, device="cuda")
    if bad != "kv_parts":
        with pytest.raises(Vq3Error):
            ops.qwen_flash_fwd(Q, K, V, mask, B, L, Hq, Hkv, D, SCALE)
        return
    O, lse = ops.qwen_flash_fwd(Q, K, V, mask, B, L, Hq, Hkv, D, SCALE)
    with pytest.raises(Vq3Error):
        ops.qwen_flash_bwd(Q, K, V, mask, O, dO, lse, B, L, Hq, Hkv, D, SCALE, kv_parts=5)


def test_qwen_flash_kv_parts_add_up(ops):
    """kv_parts 1-4 at the Stage-2 shape: every split's slabs add up to the unsplit dK / dV (per block), masked keys are 0 in every
    slab, and dQ does not depend on the split at all."""
    B, Hkv, G, L = 2, 2, 4, 4096
    Q, K, V, dO = _cuda(*_operands(B, Hkv, G, L, seed=L + B))
    mask = _mask(B, L, "stage2")
    Hq = G * Hkv
    O, lse = ops.qwen_flash_fwd(Q, K, V, mask, B, L, Hq, Hkv, D, SCALE)
    dQ1, dK1, dV1 = ops.qwen_flash_bwd(Q, K, V, mask, O, dO, lse, B, L, Hq, Hkv, D, SCALE, kv_parts=1)
    dead_key = ~mask.bool()[:, None, :].expand(B, Hkv, L)
    for parts in (2, 3, 4):
        dQp, dKp, dVp = ops.qwen_flash_bwd(Q, K, V, mask, O, dO, lse, B, L, Hq, Hkv, D, SCALE, kv_parts=parts)
        assert dKp.shape == (parts, B, Hkv, L, D)
        assert torch.equal(dQp, dQ1), parts
        for name, slabs, whole in (("dK", dKp, dK1), ("dV", dVp, dV1)):
            assert torch.isfinite(slabs.float()).all()
            assert all((slabs[i][dead_key] == 0).all() for i in range(parts)), (name, parts)
            _assert_blocks(f"{name} kv_parts={parts}", slabs.double().sum(0), whole, 1e-2)


def test_qwen_flash_is_repeatable(ops):
    """Fixed summation order (no atomics): forward + backward three times at L = 4096, padded, bit-identical."""
    B, Hkv, G, L = 2, 2, 4, 4096
    Q, K, V, dO = _cuda(*_operands(B, Hkv, G, L, seed=5))
    mask = _mask(B, L, "stage2")
    mask[0, :300] = 0
    runs = []
    for _ in range(3):
        O, lse = ops.qwen_flash_fwd(Q, K, V, mask, B, L, 4 * Hkv, Hkv, D, SCALE)
        runs.append((O, lse) + tuple(ops.qwen_flash_bwd(Q, K, V, mask, O, dO, lse, B, L, 4 * Hkv, Hkv, D, SCALE, kv_parts=2)))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)


def _front_of(t, fill, extra):
    """t's values in a view at the front of a longer allocation whose tail holds `fill`."""
    buf = torch.full((t.numel() + extra,), fill, device=t.device, dtype=t.dtype)
    v = buf[: t.numel()].view(t.shape)
    v.copy_(t)
    return buf, v


def test_qwen_flash_stays_inside_its_tensors(ops):
    """L = 1000 (a partial last tile): operands that are views at the front of NaN-filled allocations, the key mask followed by
    ones, O written through out= into a sentinel-filled buffer. Results bit-equal to exact-size tensors, the sentinel tail untouched."""
    B, Hkv, G, L = 2, 1, 4, 1000
    Hq = G * Hkv
    Q, K, V, dO = _cuda(*_operands(B, Hkv, G, L, seed=9))
    mask = _mask(B, L, "stage1")
    mask[1, :] = 1
    mask[1, 990:] = 0
    O, lse = ops.qwen_flash_fwd(Q, K, V, mask, B, L, Hq, Hkv, D, SCALE)
    dQ, dK, dV = ops.qwen_flash_bwd(Q, K, V, mask, O, dO, lse, B, L, Hq, Hkv, D, SCALE)
    nan = float("nan")
    _, Qv = _front_of(Q, nan, 64 * D)
    _, Kv = _front_of(K, nan, 64 * D)
    _, Vv = _front_of(V, nan, 64 * D)
    _, dOv = _front_of(dO, nan, 64 * Hq * D)
    _, mv = _front_of(mask, 1, 4096)
    SENT = -768.0                                         # exact in bf16
    obuf = torch.full((B * L * Hq * D + 64 * Hq * D,), SENT, device="cuda", dtype=BF16)
    Ov, lse2 = ops.qwen_flash_fwd(Qv, Kv, Vv, mv, B, L, Hq, Hkv, D, SCALE, out=obuf[: B * L * Hq * D].view(B * L, Hq * D))
    assert torch.equal(Ov, O) and torch.equal(lse2, lse)
    assert (obuf[B * L * Hq * D:] == SENT).all()
    _, Ov2 = _front_of(O, nan, 64 * Hq * D)
    g2 = ops.qwen_flash_bwd(Qv, Kv, Vv, mv, Ov2, dOv, lse2, B, L, Hq, Hkv, D, SCALE)
    for a, b in zip(g2, (dQ, dK, dV)):
        assert torch.equal(a, b)


def delta_slack_is_ignored(ops, L=1001):
    """Nothing reads past [B, Hq, L] of the backward's LSE / Delta arguments (every lane reads one float of a row clamped to L - 1):
    what lies behind them must not matter. Called straight through the C ABI with NaN behind both, at an L that is not a multiple
    of 4, against the wrapper's own call."""
    from vggt_qwen3_amd import _lib
    B, Hkv, G = 1, 1, 4
    Hq = G * Hkv
    Q, K, V, dO = _cuda(*_operands(B, Hkv, G, L, seed=13))
    mask = torch.ones(B, L, dtype=torch.uint8, device="cuda")
    O, lse = ops.qwen_flash_fwd(Q, K, V, mask, B, L, Hq, Hkv, D, SCALE)
    want = ops.qwen_flash_bwd(Q, K, V, mask, O, dO, lse, B, L, Hq, Hkv, D, SCALE)
    n = B * Hq * L
    lse_p = torch.full((n + 4,), float("nan"), device="cuda", dtype=F32)
    lse_p[:n] = lse.flatten()
    delta = torch.full((n + 4,), float("nan"), device="cuda", dtype=F32)
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    _lib.check(_lib.load().vq3_qwen_flash_bwd(Q.data_ptr(), K.data_ptr(), V.data_ptr(), mask.data_ptr(), O.data_ptr(), dO.data_ptr(),
                                              lse_p.data_ptr(), delta.data_ptr(), dQ.data_ptr(), dK.data_ptr(), dV.data_ptr(), 1, B, L,
                                              Hq, Hkv, D, O.stride(0), dO.stride(0), SCALE, torch.cuda.current_stream().cuda_stream),
               "vq3_qwen_flash_bwd")
    for name, a, b in zip("QKV", (dQ, dK, dV), want):
        assert torch.isfinite(a.float()).all(), f"d{name} not finite with NaN slack behind LSE / Delta"
        assert torch.equal(a, b), name
    ref = attn_ref64(Q, K, V, dO, mask)
    check_attention(mask, Hq, O, lse, ref, dQ, dK, dV)


def test_qwen_flash_ignores_the_slack_behind_delta(ops):
    delta_slack_is_ignored(ops)


def test_qwen_flash_holes_with_split(ops):
    """Middle key tiles dropped, dead leading rows, G = 2 (two waves idle in the head reduction) and three partial dK / dV slabs."""
    run_case(ops, 1, 2, 2, 1032, "holes", seed=1033, kv_parts=3)


# ------------------------------------------------------------------------------------------------ decode attention
@pytest.mark.parametrize("Lmax,Hq,Hkv,lens", [(4096, 32, 8, [0, 63, 64, 2000, 4095]), (12288, 16, 4, [0, 63, 64, 4095, 12287])])
def test_decode_attention_long_cache_vs_fp64(ops, Lmax, Hq, Hkv, lens):
    """qwen_decode_qkprep then qwen_decode_attn over caches of up to 12 288 rows with ragged lengths, rows past lens[b] NaN (never
    read), spiked keys - one past row 4096 of the 12 288 cache that outscores every earlier row by ~e^90 - against an fp64 softmax
    over rows 0 .. lens[b]; max abs error per (b, head)."""
    g = torch.Generator().manual_seed(Lmax)
    B = len(lens)
    G = Hq // Hkv
    lens_t = torch.tensor(lens, dtype=torch.int32, device="cuda")
    Kc = torch.randn(B, Hkv, Lmax, D, generator=g).to(BF16)
    Vc = torch.randn(B, Hkv, Lmax, D, generator=g).to(BF16)
    for b, n in enumerate(lens):
        Kc[b, :, n + 1:] = float("nan")
        Vc[b, :, n + 1:] = float("nan")
    Kc, Vc = Kc.cuda(), Vc.cuda()
    qkv = torch.randn(B, (Hq + 2 * Hkv) * D, generator=g).to(BF16).cuda()
    qw = (1 + 0.2 * torch.randn(D, generator=g)).to(BF16).cuda()
    kw = (1 + 0.2 * torch.randn(D, generator=g)).to(BF16).cuda()
    ang = torch.rand(Lmax, D // 2, generator=g) * 6.28
    emb = torch.cat([ang, ang], -1)
    cos, sin = emb.cos().to(BF16).cuda().contiguous(), emb.sin().to(BF16).cuda().contiguous()
    Q = ops.qwen_decode_qkprep(qkv, qw, kw, cos, sin, lens_t, Kc, Vc, B, Hq, Hkv, D, Lmax, 1e-6)
    Qh = Q.view(B, Hq, D)
    # spikes (row j of kv head h // G = f x the query of head h): planted after qkprep, which writes row lens[b] and the queries
    spikes = [(B - 1, lens[-1] - 3, 1, 5.0), (3, lens[3] // 2, G, 6.0), (2, 0, 0, 4.0)]
    if Lmax > 4096:
        spikes.append((B - 1, 9000, Hq - 1, 8.5))
    for b, j, h, f in spikes:
        Kc[b, h // G, j] = (f * Qh[b, h].float()).to(BF16)
    O = ops.qwen_decode_attn(Q, Kc, Vc, lens_t, B, Hq, Hkv, D, Lmax, SCALE).view(B, Hq, D)
    assert torch.isfinite(O.float()).all()
    for b, n in enumerate(lens):
        T = n + 1
        k = Kc[b, :, :T].double().repeat_interleave(G, 0)           # [Hq, T, D]
        v = Vc[b, :, :T].double().repeat_interleave(G, 0)
        s = torch.einsum("hd,htd->ht", Qh[b].double(), k) * SCALE
        ref = torch.einsum("ht,htd->hd", torch.softmax(s, -1), v)
        err = (O[b].double() - ref).abs().amax(-1)
        bound = 2e-2 * ref.abs().amax(-1).clamp_min(1.0)
        assert (err <= bound).all(), (b, n, int((err / bound).argmax()), float((err / bound).max()))
    for b, j, h, f in spikes:
        if f > 6.0:                                               # saturated: the output is that key's value row
            assert (O[b, h].float() - Vc[b, h // G, j].float()).abs().max().item() < 2e-2


@pytest.mark.parametrize("Lmax", [63, 12289])
def test_decode_attention_rejects_cache_capacity(ops, Lmax):
    from vggt_qwen3_amd._lib import Vq3Error
    Q = torch.zeros(1, 4 * D, device="cuda", dtype=BF16)
    Kc = torch.zeros(1, 1, 64, D, device="cuda", dtype=BF16)
    lens = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(Vq3Error):
        ops.qwen_decode_attn(Q, Kc, Kc, lens, 1, 4, 1, D, Lmax, SCALE)
