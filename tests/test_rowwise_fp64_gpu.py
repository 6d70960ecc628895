"""The row-wise kernels between the Qwen3 GEMMs against the fp64 restatements of tests/rowwise_ref.py, on every dispatch branch.

All references run in fp64 on the device from the operands the kernels read; every comparison is made tight and loose (see
rowwise_ref.py for the two forms and for every bound's derivation). `pytest -s` prints the TOL lines. Every buffer a kernel writes sits
between guard bands of a sentinel that must come back bit-unchanged; strided rows carry the sentinel in their slack columns and NaN in
the input's. Where the Python wrapper allocates an output itself (rmsnorm rstd, LayerNorm y / dx and its partial rows, q/k-prep Q / K /
V / rstd, SwiGLU dgu) the same kernel is driven through its C entry with guarded buffers and the wrapper's result must equal it bit for
bit; AdamW's p / m / v live in guarded slabs.

Case -> branch:
  test_rmsnorm[cols]        cols 8..512 -> rmsnorm_bwd_kernel<1, *>, 520..1024 -> <2, *>, 1032..2560 -> <5, *>, 2568, 4096 -> <8, *>;
                            rows 1, 3, 5, 1201 -> a last workgroup with 1-3 live waves (rows % 4 != 0), ldx / ldy = cols + 8, + 264;
                            VQ3_RMSNORM_BWD_ROWS 4 -> RB = 4, 8 / 16 / 256 -> the RB = 0 run-time path; the raw vq3_rmsnorm_bwd entry;
                            dres None / given; accumulate; defer= + colsum_flush bit-identical to the direct column sum
  test_colsum[nrows]        nrows 1..130 -> the r + 48 < nrows loop against its tail; 1024 / 1025 / 9600 -> nsplit 2 / 2 / 18 and the ticket
                            clear (two launches in a row); cols 8, 72 -> cols % 64 != 0; 8 jobs of different cols -> the early return;
                            nrows 1, 17, 130 at cols 8, 200 -> colsum_kernel<float> rounded to bf16 == colsum_kernel<bf16_t> (one body)
  test_layernorm_fwd[cols]  4..1024 -> NCH 4, 1028..2048 -> 8, 4096 -> 16, 4100 / 8192 -> generic NCH 0; 252, 1028, 4100 -> cols % 256 != 0
  test_layernorm_bwd[cols]  4..1024 -> NCH 4, 2048 -> 8, 4096 -> 16; rows 1, 13, 17, 19, 1029 -> rows % 16 in 1..3 and waves that break early
  test_qkprep[case]         (32, 8, 2, 301): Qwen3-4B heads, B L % 8 = 2 -> the t >= T break; (5, 3, 1, 33) and (1, 1, 3, 5): odd HT, the
                            half-waves disagree; (64, 8, 1, 19), (40, 8, 1, 9): HT > 48, a second trip of the hb loop; (4, 1, 1, 12288): long
                            tables; kv_parts 1-4 -> the sp loop; want_rstd=False
  test_swiglu[shape]        (1, 8): inter = 8; (9600, 9728): past the flat_grid cap (2048 workgroups), the grid-stride loop; saturated gates
  test_adamw[n]             n 1, 3 -> n < 4 (tail only); 4, 5, 1023, 1024, 1000003 -> n % 4 in 0..3; step 100000 -> bc2_sqrt ~ 1; gscale + clip
  test_sumsq                bf16 n % 8 != 0, f32 n % 4 != 0, accumulator starts non-zero, two calls accumulate, bit-repeatable

Modes that are paired with a case, not crossed with every case: test_qkprep runs kv_parts 1 and 3 with accumulate=False and 2 and 4 with
accumulate=True; test_layernorm_bwd accumulates into dw_out / db_out at rows 1, 16 and 19 and lets the wrapper allocate at 13, 17 and
1029; test_layernorm_fwd cycles (both outputs, bf16 only, f32 only) over its (rows, dtype, res) cases; test_rmsnorm runs all five
backward modes at rows 5 and 1201 and one at the others; swiglu (1, 8) holds only the first 8 edge combinations (gate +0.0), the other
shapes hold all 256.

SwiGLU d_gate: every edge combination whose fp64 value is finite in bf16 is asserted finite and compared. With dact = up = +-3e38 and a
saturated negative gate the kernel once formed dact * up = inf first and returned inf * 0 = NaN for a true 0; swiglu_dgate_f now
multiplies the bounded factor in first."""
import math

import pytest
import torch

from tests import rowwise_ref as R
from tests.rowwise_ref import BF16, F32, F64

pytestmark = pytest.mark.gpu
EPS = 1e-6
SENT = 777.0
BAND = 4096


@pytest.fixture(scope="module")
def ops():
    from vggt_qwen3_amd import _lib
    from vggt_qwen3_amd import ops as _ops
    _lib.load()
    return _ops


@pytest.fixture(scope="module")
def lib():
    from vggt_qwen3_amd import _lib
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def rnd(shape, seed, scale=1.0, dtype=BF16):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(shape, generator=g, device="cuda") * scale).to(dtype)


class Guard:
    """A [rows, cols] view with row stride ld inside a buffer of sentinels: a band before, a band after, the slack columns."""

    def __init__(self, rows, cols, dtype=BF16, ld=None, fill=None):
        self.rows, self.cols, self.ld = rows, cols, ld or cols
        self.buf = torch.full((2 * BAND + rows * self.ld,), SENT, device="cuda", dtype=dtype)
        self.body = self.buf[BAND:BAND + rows * self.ld].view(rows, self.ld)
        self.t = self.body[:, :cols]
        if fill is not None:
            self.t.copy_(fill)

    def check(self, tag):
        ok = (self.buf[:BAND] == SENT).all() and (self.buf[-BAND:] == SENT).all() and (self.body[:, self.cols:] == SENT).all()
        assert ok, tag + ": guard band or slack columns overwritten"


def vec(g):
    return g.t.view(-1) if g.ld == g.cols else g.t.reshape(-1)


# ================================================================================================ RMSNorm
def rms_rows(rows, cols, seed):
    """Row kinds inside one tensor: N(0, 2), all-zero, magnitude 1e4, 1e-20 (the squares underflow), one spike of 3e4 among zeros."""
    x = rnd((rows, cols), seed, 2.0, F32)
    for r0 in range(0, rows - 4, 600):
        x[r0 + 1] = 0
        x[r0 + 2] *= 1e4
        x[r0 + 3] *= 1e-20
        x[r0 + 4] = 0
        x[r0 + 4, cols // 2] = 3e4
    if rows == 1:
        x[0, 1:] = 0
    return x.to(BF16)


def run_rmsnorm(ops, lib, monkeypatch, rows, cols, full):
    from vggt_qwen3_amd._lib import check
    tag = f"rmsnorm {rows}x{cols}"
    x, w = rms_rows(rows, cols, cols + rows), (1 + rnd((cols,), 2, 0.2, F32)).to(BF16)
    y0 = rs0 = None
    for pad in (0, 8, 264):
        xs = torch.full((rows, cols + pad), float("nan"), device="cuda", dtype=BF16)
        xs[:, :cols] = x
        g = Guard(rows, cols, ld=cols + pad)
        y, rs = ops.rmsnorm_fwd(xs[:, :cols], w, EPS, want_rstd=True, out=g.t)
        g.check(tag)
        R.check_rmsnorm_fwd(f"{tag} ld+{pad}", y, rs, x, w, EPS)
        g2, gr = Guard(rows, cols, ld=cols + pad), Guard(1, rows, dtype=F32)          # the C entry: rstd between guard bands too
        check(lib.vq3_rmsnorm_fwd(xs.data_ptr(), w.data_ptr(), g2.t.data_ptr(), gr.t.data_ptr(), rows, cols, cols + pad, cols + pad, EPS,
                                  stream()), "vq3_rmsnorm_fwd")
        g2.check(tag)
        gr.check(tag)
        assert torch.equal(g2.t, y) and R.bits_equal(vec(gr), rs), "wrapper and C entry must give the same bits"
        if y0 is None:
            y0, rs0 = y.clone(), rs
        assert torch.equal(y, y0) and torch.equal(rs, rs0), "strided rows must give the same bits"
    zero = (x == 0).all(1)
    assert torch.allclose(rs0[zero], torch.full_like(rs0[zero], EPS ** -0.5), rtol=1e-6)
    dy, dres = rnd((rows, cols), 3), rnd((rows, cols), 4)
    modes = [(4, dres, False), (4, None, True), (8, None, False), (16, dres, True), (256, dres, False)] if full else [(4, dres, True)]
    for rpp, dr, acc in modes:
        monkeypatch.setenv("VQ3_RMSNORM_BWD_ROWS", str(rpp))
        old = rnd((1, cols), 5)
        gdx, gdw = Guard(rows, cols), Guard(1, cols, fill=old)
        ops.rmsnorm_bwd(dy, x, w, rs0, dr, vec(gdw), acc, out=gdx.t)
        gdx.check(tag)
        gdw.check(tag)
        t2 = f"{tag} rpp={rpp}"
        R.check_rmsnorm_bwd_dx(t2, gdx.t, dy, x, w, rs0, dr)
        R.check_rmsnorm_bwd_dw(t2, vec(gdw), dy, x, rs0, rpp, old=old[0] if acc else None)
        if dr is None:
            z = gdx.t[zero].double()
            assert torch.isfinite(z).all() and torch.equal(gdx.t[zero], (rs0[zero, None] * (dy[zero].float() * w.float())).to(BF16))
        # the deferred column sum gives the same bits
        jobs, old2 = [], Guard(1, cols, fill=old)
        dx2 = ops.rmsnorm_bwd(dy, x, w, rs0, dr, vec(old2), acc, defer=jobs)
        ops.colsum_flush(jobs)
        old2.check(tag)
        assert torch.equal(dx2, gdx.t) and torch.equal(old2.t, gdw.t), "defer= + colsum_flush must be bit-identical to the direct column sum"
    # monkeypatch restores the variable at teardown; it is dropped here so that what follows in this helper runs with the default of 4
    monkeypatch.delenv("VQ3_RMSNORM_BWD_ROWS", raising=False)
    # the raw vq3_rmsnorm_bwd entry: 4 rows per partial
    nblk = (rows + 3) // 4
    gdx, part = Guard(rows, cols), Guard(nblk, cols, dtype=F32)
    check(lib.vq3_rmsnorm_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(), rs0.data_ptr(), None, gdx.t.data_ptr(), part.t.data_ptr(), rows,
                              cols, EPS, stream()), "vq3_rmsnorm_bwd")
    gdx.check(tag)
    part.check(tag)
    R.check_rmsnorm_bwd_dx(tag + " raw", gdx.t, dy, x, w, rs0, None)
    terms = dy.double() * x.double() * rs0.double()[:, None]
    pad = torch.zeros(nblk * 4, cols, device="cuda", dtype=F64)
    pad[:rows] = terms
    R.check_colsum(tag + " raw dw partial rows", part.t.reshape(-1), pad.view(nblk, 4, cols).transpose(0, 1).reshape(4, -1), 3 + 2,
                   out_bf16=False)


@pytest.mark.parametrize("cols", [8, 128, 512, 520, 1024, 1032, 2560, 2568, 4096])
def test_rmsnorm(ops, lib, monkeypatch, cols):
    for rows in (1, 3, 4, 5, 1201):
        run_rmsnorm(ops, lib, monkeypatch, rows, cols, full=rows in (5, 1201))


def test_rmsnorm_merged_pass_shape(ops, lib, monkeypatch):
    run_rmsnorm(ops, lib, monkeypatch, 9600, 2560, full=False)


def test_rmsnorm_fwd_rejects_bad_out(ops):
    from vggt_qwen3_amd._lib import Vq3Error
    x, w = rnd((4, 128), 1), rnd((128,), 2)
    with pytest.raises(Vq3Error):
        ops.rmsnorm_fwd(x, w, EPS, out=torch.empty((4, 136), device="cuda", dtype=F32)[:, :128])
    with pytest.raises(Vq3Error):                      # the C entry's argument check on ldy % 8
        ops.rmsnorm_fwd(x, w, EPS, out=torch.empty((4, 132), device="cuda", dtype=BF16)[:, :128])      # row stride not a multiple of 8


# ================================================================================================ column sums
CS_COLS = [8, 64, 72, 128, 2560, 4096]


@pytest.mark.parametrize("nrows", [1, 15, 16, 17, 48, 49, 63, 64, 65, 113, 130, 1023, 1024, 1025, 9600])
def test_colsum(ops, lib, nrows):
    from vggt_qwen3_amd._lib import check
    gi = torch.Generator(device="cuda").manual_seed(nrows)
    for acc in (False, True):
        jobs, expect, guards = [], [], []
        for k, cols in enumerate(CS_COLS + [64, 128]):
            nr = nrows if k < 6 else nrows // 2 + 1
            # integers in [-8, 8]: every f32 partial sum is exact (|sum| <= 76 800 < 2^24), so the result must be bf16(sum) exactly
            part = torch.randint(-8, 9, (nr, cols), generator=gi, device="cuda").float()
            old = torch.randint(-8, 9, (1, cols), generator=gi, device="cuda").to(BF16)
            want = (part.double().sum(0) + (old[0].double() if acc else 0)).to(BF16)
            tag = f"colsum {nr}x{cols} acc={acc}"
            g = Guard(1, cols, fill=old)
            check(lib.vq3_colsum_f32_to_bf16(part.data_ptr(), nr, cols, g.t.data_ptr(), int(acc), stream()), "colsum")
            g.check(tag)
            assert torch.equal(g.t[0], want), tag + ": vq3_colsum_f32_to_bf16 is not exact on integers"
            gf = Guard(1, cols, dtype=F32, fill=old.float())
            check(lib.vq3_colsum_f32(part.data_ptr(), nr, cols, gf.t.data_ptr(), int(acc), stream()), "colsum_f32")
            gf.check(tag)
            assert torch.equal(gf.t[0].double(), part.double().sum(0) + (old[0].double() if acc else 0)), tag + ": vq3_colsum_f32 not exact"
            gm = Guard(1, cols, fill=old)
            jobs.append((part, nr, cols, vec(gm), acc)); expect.append(want); guards.append(gm)
        # two launches in a row on one stream. vq3_colsum_multi clears the arrival tickets with a memset before every launch, so this
        # pins that a second split launch right behind the first is still exact, not the kernel's own ticket reset
        for rep in range(2):
            for gm, (_, _, cols, _, _) in zip(guards, jobs):
                gm.t.copy_(torch.randint(-8, 9, (1, cols), generator=gi, device="cuda").to(BF16)) if rep else None
            olds = [gm.t[0].double().clone() for gm in guards]
            ops.colsum_flush(list(jobs))
            for gm, (part, nr, cols, _, _), o in zip(guards, jobs, olds):
                gm.check(f"colsum_multi {nr}x{cols}")
                want = (part.double().sum(0) + (o if acc else 0)).to(BF16)
                assert torch.equal(gm.t[0], want), f"colsum_multi {nr}x{cols} acc={acc} launch {rep}: not exact on integers"
    # one random case per shape against fp64
    for cols in CS_COLS:
        part, old = rnd((nrows, cols), nrows + cols, 1.0, F32), rnd((1, cols), 7)
        g = Guard(1, cols, fill=old)
        ops.colsum_flush([(part, nrows, cols, vec(g), True)])
        g.check("colsum random")
        R.check_colsum(f"colsum random {nrows}x{cols}", g.t[0], part, R.colsum_depth(nrows), old=old[0])
        gf = Guard(1, cols, dtype=F32)
        ops.colsum_f32(part, out=vec(gf))
        gf.check("colsum_f32 random")
        R.check_colsum(f"colsum_f32 random {nrows}x{cols}", vec(gf), part, R.colsum_depth(nrows), out_bf16=False)
    # the f32 and the bf16 entry are one body: the same additions in the same order, one round-to-nearest-even at the end
    if nrows in (1, 17, 130):
        for cols in (8, 200):
            part = rnd((nrows, cols), nrows + cols, 1.0, F32)
            g = Guard(1, cols)
            check(lib.vq3_colsum_f32_to_bf16(part.data_ptr(), nrows, cols, g.t.data_ptr(), 0, stream()), "colsum")
            g.check("colsum one body")
            assert torch.equal(ops.colsum_f32(part).to(BF16), g.t[0]), f"colsum {nrows}x{cols}: bf16(vq3_colsum_f32) != vq3_colsum_f32_to_bf16"


# ================================================================================================ LayerNorm
@pytest.mark.parametrize("cols", [4, 252, 256, 1024, 1028, 2048, 4096, 4100, 8192])
def test_layernorm_fwd(ops, lib, cols):
    from vggt_qwen3_amd._lib import check
    w, b = 1 + rnd((cols,), 9, 0.2, F32), rnd((cols,), 10, 0.2, F32)
    k = 0
    for rows in (1, 5, 770):
        shift = torch.tensor([0.0, 1e3] * rows, device="cuda")[:rows, None]          # rows of mean 1e3, std 1: cancellation
        for dt in (F32, BF16):
            x = (rnd((rows, cols), 11 + rows, 1.0, F32) + shift).to(dt)
            for res in (None, rnd((rows, cols), 12, 1.0, dt)):
                wb, wf = [(True, True), (True, False), (False, True)][k % 3]
                k += 1
                yb, yf = ops.layernorm_fwd(x, w, b, EPS, res=res, want_bf16=wb, want_f32=wf)
                assert (yb is None) == (not wb) and (yf is None) == (not wf)
                gb, gf = Guard(rows, cols), Guard(rows, cols, dtype=F32)          # the C entry writes between guard bands
                check(lib.vq3_layernorm_fwd(x.data_ptr(), None if res is None else res.data_ptr(), int(dt == F32), w.data_ptr(), b.data_ptr(),
                                            gb.t.data_ptr() if wb else None, gf.t.data_ptr() if wf else None, rows, cols, EPS, stream()),
                      "vq3_layernorm_fwd")
                gb.check("layernorm_fwd")
                gf.check("layernorm_fwd")
                assert (gb.t == SENT).all() if not wb else R.bits_equal(gb.t, yb), "an output not asked for is not written"
                assert (gf.t == SENT).all() if not wf else R.bits_equal(gf.t, yf)
                R.check_layernorm_fwd(f"layernorm_fwd {rows}x{cols} {dt} res={res is not None}", yb, yf, x, res, w, b, EPS)


@pytest.mark.parametrize("cols", [4, 256, 1024, 2048, 4096])
def test_layernorm_bwd(ops, lib, cols):
    from vggt_qwen3_amd._lib import check
    w = 1 + rnd((cols,), 9, 0.2, F32)
    for i, rows in enumerate((1, 13, 16, 17, 19, 1029)):
        x, res, dy = rnd((rows, cols), 13, 1.0, F32) + 3, rnd((rows, cols), 14, 1.0, F32), rnd((rows, cols), 15, 1.0, F32)
        for r in (None, res):
            outs = i % 2 == 0
            dw0, db0 = rnd((cols,), 16, 1.0, F32), rnd((cols,), 17, 1.0, F32)
            gw, gb = Guard(1, cols, dtype=F32, fill=dw0[None]), Guard(1, cols, dtype=F32, fill=db0[None])
            dx, dw, db = ops.layernorm_bwd(dy, x, w, EPS, res=r, dw_out=vec(gw) if outs else None, db_out=vec(gb) if outs else None)
            gw.check("layernorm_bwd")
            gb.check("layernorm_bwd")
            nblk = (rows + 15) // 16                                              # the C entry: dx and the partial rows between guard bands
            gdx, gp = Guard(rows, cols, dtype=F32), Guard(2 * nblk, cols, dtype=F32)
            check(lib.vq3_layernorm_bwd(dy.data_ptr(), x.data_ptr(), None if r is None else r.data_ptr(), w.data_ptr(), gdx.t.data_ptr(),
                                        gp.t[:nblk].data_ptr(), gp.t[nblk:].data_ptr(), rows, cols, EPS, stream()), "vq3_layernorm_bwd")
            gdx.check("layernorm_bwd dx")
            gp.check("layernorm_bwd partial rows")
            assert R.bits_equal(gdx.t, dx), "wrapper and C entry must give the same dx"
            R.check_colsum("layernorm_bwd db partial rows", gp.t[nblk:].sum(0, dtype=F64), dy, 4 + 3, out_bf16=False)      # 4 rows per wave, 3 adds across the waves
            R.check_layernorm_bwd(f"layernorm_bwd {rows}x{cols} res={r is not None}", dx, dw, db, dy, x, r, w, EPS,
                                  dw_old=dw0 if outs else None, db_old=db0 if outs else None)


# ================================================================================================ QK-norm + RoPE
QK_CASES = [(32, 8, 2, 301), (8, 2, 1, 7), (1, 1, 3, 5), (5, 3, 1, 33), (64, 8, 1, 19), (40, 8, 1, 9), (4, 1, 1, 12288)]


@pytest.mark.parametrize("Hq,Hkv,B,L", QK_CASES)
def test_qkprep(ops, lib, Hq, Hkv, B, L):
    from vggt_qwen3_amd._lib import check
    D, HT = 128, Hq + 2 * Hkv
    tag = f"qkprep Hq={Hq} Hkv={Hkv} B={B} L={L}"
    qkv = rnd((B * L, HT * D), 20, 1.5)
    qw, kw = (1 + rnd((D,), 21, 0.3, F32)).to(BF16), (1 + rnd((D,), 22, 0.3, F32)).to(BF16)
    cos, sin = R.rope_tables(L, device="cuda")
    Q, K, V, qr, kr = ops.qwen_qkprep_fwd(qkv, qw, kw, cos, sin, B, L, Hq, Hkv, D, EPS)
    T = B * L                                                                     # the C entry: every output between guard bands
    gQ, gK, gV = Guard(1, T * Hq * D), Guard(1, T * Hkv * D), Guard(1, T * Hkv * D)
    gqr, gkr = Guard(1, T * Hq, dtype=F32), Guard(1, T * Hkv, dtype=F32)
    check(lib.vq3_qwen_qkprep_fwd(qkv.data_ptr(), qw.data_ptr(), kw.data_ptr(), cos.data_ptr(), sin.data_ptr(), gQ.t.data_ptr(),
                                  gK.t.data_ptr(), gV.t.data_ptr(), gqr.t.data_ptr(), gkr.t.data_ptr(), B, L, Hq, Hkv, D, EPS, stream()),
          "vq3_qwen_qkprep_fwd")
    for g, ref in ((gQ, Q), (gK, K), (gV, V), (gqr, qr), (gkr, kr)):
        g.check(tag)
        assert R.bits_equal(vec(g), ref.reshape(-1)), "wrapper and C entry must give the same bits"
    R.check_qkprep_fwd(tag, Q, K, V, qr, kr, qkv, qw, kw, cos, sin, B, L, Hq, Hkv, EPS)
    Q2, K2, V2, n1, n2 = ops.qwen_qkprep_fwd(qkv, qw, kw, cos, sin, B, L, Hq, Hkv, D, EPS, want_rstd=False)
    assert n1 is None and n2 is None and torch.equal(Q2, Q) and torch.equal(K2, K) and torch.equal(V2, V)
    dQ = rnd((B, Hq, L, D), 23)
    for parts in (1, 2, 3, 4):
        # the slab split is made here, so the fp64 sum of the slabs is known: independent random slabs
        dK, dV = rnd((parts, B, Hkv, L, D), 24 + parts), rnd((parts, B, Hkv, L, D), 28 + parts)
        acc = parts % 2 == 0
        oq, ok_ = rnd((1, D), 32), rnd((1, D), 33)
        gq, gk, gx = Guard(1, D, fill=oq), Guard(1, D, fill=ok_), Guard(B * L, HT * D)
        out = ops.qwen_qkprep_bwd(dQ, dK if parts > 1 else dK[0], dV if parts > 1 else dV[0], qkv, qw, kw, cos, sin, qr, kr, vec(gq), vec(gk),
                                  acc, B, L, Hq, Hkv, D, out=gx.t)
        for g in (gq, gk, gx):
            g.check(tag)
        R.check_qkprep_bwd(f"{tag} parts={parts}", out, vec(gq), vec(gk), dQ, dK, dV, qkv, qw, kw, cos, sin, qr, kr, B, L, Hq, Hkv,
                           old_q=oq[0] if acc else None, old_k=ok_[0] if acc else None)


# ================================================================================================ SwiGLU
def swiglu_case(rows, inter, seed):
    """N(0, 1.5), and in the first elements every edge gate against every edge up / dact value."""
    gu, dact = rnd((rows, 2 * inter), seed, 1.5, F32), rnd((rows, inter), seed + 1, 1.0, F32)
    gates = [0.0, -0.0, 1e-30, -1e-30, 20, -20, 87, -87, 89, -89, 200, -200, 3e38, -3e38, R.BF16_MAX, -R.BF16_MAX]
    edge = [0.0, 3e38, -3e38, 1.0]
    combos = [(a, b_, c) for a in gates for b_ in edge for c in edge]
    n = min(len(combos), rows * inter)
    t = torch.tensor(combos[:n], device="cuda", dtype=F32)
    idx = torch.arange(n, device="cuda")
    r, c = idx // inter, idx % inter
    gu[r, c], gu[r, inter + c], dact[r, c] = t[:, 0], t[:, 1], t[:, 2]
    return gu.to(BF16), dact.to(BF16)


@pytest.mark.parametrize("rows,inter", [(1, 8), (3, 136), (300, 9728), (9600, 9728)])
def test_swiglu(ops, lib, rows, inter):
    from vggt_qwen3_amd._lib import check
    if rows == 9600:
        assert rows * (inter // 8) > 2048 * 256, "this shape must cross the flat_grid cap (2048 workgroups of 256 threads)"
    gu, dact = swiglu_case(rows, inter, 30)
    g = Guard(rows, inter)
    act = ops.silu_mul_fwd(gu, out=g.t)
    g.check("swiglu")
    dgu = ops.silu_mul_bwd(dact, gu)
    gd = Guard(rows, 2 * inter)                                                   # the C entry: dgu between guard bands
    check(lib.vq3_silu_mul_bwd(dact.data_ptr(), gu.data_ptr(), gd.t.data_ptr(), rows, inter, stream()), "vq3_silu_mul_bwd")
    gd.check("swiglu dgu")
    assert R.bits_equal(gd.t, dgu), "wrapper and C entry must give the same bits"
    del gd
    step = 2400 if rows == 9600 else rows          # fp64 in row blocks
    for r0 in range(0, rows, step):
        sl = slice(r0, r0 + step)
        R.check_silu_mul_fwd(f"swiglu {rows}x{inter}", act[sl], gu[sl])
        R.check_silu_mul_bwd(f"swiglu {rows}x{inter}", dgu[sl], dact[sl], gu[sl])


def test_swiglu_gemm_epilogue_equals_two_launches_on_saturated_gates(ops):
    """x = I, W = gu^T: the GEMM hands the saturated gate | up values to its epilogue exactly."""
    M = H = 256
    I = 384
    gu, _ = swiglu_case(M, I, 31)
    x = torch.eye(M, device="cuda", dtype=BF16)
    W = gu.t().contiguous()                                   # [2 I, H]
    ops.gemm_force_config(20)
    try:
        gu_ref = ops.linear(x, W)
        act_ref = ops.silu_mul_fwd(gu_ref)
        gu2, act = ops.gemm_swiglu_fwd(x, W)
    finally:
        ops.gemm_force_config(-3)
    assert torch.equal(gu_ref, gu), "the identity GEMM must hand the values over unchanged"
    assert R.bits_equal(gu2, gu_ref) and R.bits_equal(act, act_ref)
    R.check_silu_mul_fwd("swiglu epilogue", act, gu_ref)


# ================================================================================================ AdamW, sum of squares
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1000003])
def test_adamw(ops, n):
    for step0 in (1, 100000):
        for wd, gscale, clip in ((0.0, 1.0, None), (0.1, 0.125, 1e9), (0.1, 1.0, 0.5), (0.0, 0.125, 0.01)):
            grad = rnd((n,), 41, 0.1)
            grad[:1] = 0
            # p, m and v are updated in place: each lives between guard bands, like w
            gp, gm, gv, gw = Guard(1, n, dtype=F32, fill=rnd((1, n), 40, 1.0, F32)), Guard(1, n, dtype=F32), Guard(1, n, dtype=F32), Guard(1, n)
            p, m, v = vec(gp), vec(gm), vec(gv)
            m.zero_(); v.zero_()
            if step0 > 1:
                m.copy_(rnd((n,), 42, 0.05, F32)); v.copy_(rnd((n,), 43, 0.05, F32).pow(2))
            ref = R.AdamW64(p, m, v, 1e-3, 0.9, 0.999, 1e-8, wd)
            sq = None
            if clip is not None:
                sq = torch.full((1,), 0.0, device="cuda", dtype=F32)
                ops.sumsq(grad, torch.empty(1024, device="cuda", dtype=F32), sq)
                coef = clip / (math.sqrt(sq.item()) * gscale + 1e-6)
                assert n < 1023 or (coef < 1) == (clip < 1e9), "the clip must be active exactly where the case says"
            for t in range(step0, step0 + 4):
                ops.adamw_step(p, m, v, grad, vec(gw), 1e-3, 0.9, 0.999, 1e-8, wd, t, gscale, None if clip is None else (sq, clip))
                for g in (gp, gm, gv, gw):
                    g.check("adamw")
                ref.step(grad, t, gscale, None if sq is None else sq.item(), clip or 0.0)
                ref.check(f"adamw n={n} step0={step0} wd={wd} gscale={gscale} clip={clip}", p, m, v, vec(gw))


@pytest.mark.parametrize("dt,n", [(BF16, 1), (BF16, 1023), (BF16, 1000003), (F32, 3), (F32, 1025), (F32, 1000003)])
def test_sumsq(ops, dt, n):
    x = rnd((n,), 50, 1.0, dt)
    gpart, gacc = Guard(1, 1024, dtype=F32), Guard(1, 1, dtype=F32, fill=torch.full((1, 1), 2.5, device="cuda"))
    part, acc = vec(gpart), vec(gacc)                                        # the kernel adds to what is there
    ops.sumsq(x, part, acc)
    gpart.check("sumsq partials")
    gacc.check("sumsq")
    first = acc.clone()
    R.check_sumsq(f"sumsq {dt} n={n}", acc.item(), x, 2.5)
    ops.sumsq(x, part, acc)                                                  # two calls accumulate
    R.check_sumsq(f"sumsq {dt} n={n} twice", acc.item(), torch.cat([x, x]), 2.5)
    again = torch.full((1,), 2.5, device="cuda", dtype=F32)
    ops.sumsq(x, part, again)
    assert R.bits_equal(again, first), "sumsq must be bit-identical across runs"
