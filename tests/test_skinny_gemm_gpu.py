"""The decode skinny GEMMs (skinny_gemm.hip: vq3_skinny_gemm_bf16, vq3_skinny_gemm_fp8) on every instantiation the dispatcher can reach,
at the smallest shapes that select it.

Dispatch (skinny_gemm.hip: plan_bf16 / plan_fp8). bf16: MT = 1, 2, 4, 8 for M = 1, 2, 3-4, 5-8. MT <= 2 with at most 20 chunks of 512
takes the register-resident kernel, KS = 1 / 2 / 4 for <= 5 / 10 / 20 chunks, and R = 4 / 2 / 1 for N >= 1024 / >= 512 / below when
xmode != 0 or N * KS >= 8192, else R = 1. MT <= 2 with more chunks takes the generic kernel with R = 4 / 2 / 1 for N >= 16384 / >= 4096 /
below; MT = 4 and 8 always take the generic kernel with R = 4. e4m3: M = 1, 2, R = 4, KS = 1 / 2 / 4 for <= 3 / 6 / more chunks of 1024.

Case -> instantiation (every case runs M and xmode as listed, with and without a residual; bf16 cases with bf16 and fp32 output):
  test_bf16_rows_1_2[520]    2 chunks  -> regx<MT, R, 1, X>: N 37 -> R 1 (X 0-2); 520 -> R 2 (X 1, 2), R 1 (X 0); 1030 -> R 4 (X 1, 2),
                                          R 1 (X 0); 8200 -> R 4 (X 0-2)
  test_bf16_rows_1_2[3080]   7 chunks  -> regx<MT, R, 2, X>: the same N with 4100 for the last
  test_bf16_rows_1_2[5640]   12 chunks -> regx<MT, R, 4, X>: the same N with 2050 for the last
  test_bf16_rows_1_2[10248]  21 chunks -> generic<MT, R, X>: N 37 -> R 1, 4100 -> R 2, 16390 -> R 4
  test_bf16_rows_3_to_8      K 520, N 37 and 1030, M 3, 4 -> generic<4, 4, X>, M 5, 8 -> generic<8, 4, X>
  test_fp8[K]                1040 / 4112 / 7184 and 2560 / 4096 / 9728 -> fp8<MT, 4, 1 / 2 / 4, X>; N 37 and 1030
520, 3080, 5640, 1040, 4112 and 7184 are no multiple of the chunk: the clamped tail load and the zeroed chunks past K; 10248 leaves the
generic kernel an 8-element tail. 37, 1030, 2050, 4100, 8200 and 16390 are no multiple of the rows per workgroup. M = 3 and 5 leave rows of
the MT tile unused. 9728 is 10 chunks of 1024 (the dispatcher's last branch).

What is asserted. xmode 0, bf16: against the fp64 product of the bf16 operands, bound derived in bound_bf16(). xmode 1 and 2: bit-equal to
ops.rmsnorm_fwd / ops.silu_mul_fwd feeding the xmode 0 product of the same (M, N, K), which holds because a row's fp32 summation order does
not depend on R. e4m3: relative Frobenius error below 3e-3 against ops.linear_fp8 fed by the stand-alone kernels (the criterion of
test_fp8_skinny_matches_fp8_gemm_contract). vq3_gemm_fp8_nt needs K % 128 == 0, so for the other K the prepared row and the quantised
weight are zero-padded to the next multiple: zeros change neither the row's amax nor the sum. Every output is written through the C entry
into a buffer with sentinel bands before and after and sentinel slack columns (ldy = N + 8), which must come back unchanged; the fp8
wrapper, which allocates its own output, must give the same bits. `pytest -s` prints the worst error / bound ratio per case."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EPS = 1e-6
SENT = 777.0
BAND = 4096
KMAX, NMAX = 10248, 16390
# K -> the N that select each R (see the module docstring)
BF16_CASES = {520: (37, 520, 1030, 8200), 3080: (37, 520, 1030, 4100), 5640: (37, 520, 1030, 2050), 10248: (37, 4100, 16390)}
FP8_K = (1040, 4112, 7184, 2560, 4096, 9728)
FP8_N = (37, 1030)


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


class Data:
    """Operands created once per module; every case reads a leading block of them. The fp64 references are computed once per K."""

    def __init__(self):
        self.W = rnd((NMAX, KMAX), 1, 0.05)                       # 336 MB; a case's weight is W[:N, :K] with ldw = KMAX
        self.x = rnd((8, KMAX), 2)
        self.gu = rnd((8, 2 * KMAX), 3)
        self.lnw = (1 + rnd((KMAX,), 4, 0.2, F32)).to(BF16)
        self.res = rnd((8, NMAX), 5)
        self.W8 = rnd((max(FP8_N), max(FP8_K)), 6, 0.03)
        self._ref = {}

    def ref(self, K, nmax):
        """(x W^T, |x| |W|^T) in fp64 for the 8 rows of x[:, :K] and the first nmax rows of W[:, :K]."""
        if K not in self._ref:
            x, w = self.x[:, :K].double(), self.W[:nmax, :K].double()
            self._ref[K] = (x @ w.t(), x.abs() @ w.abs().t())
        return self._ref[K]


@pytest.fixture(scope="module")
def data():
    return Data()


class Guard:
    """A [rows, cols] view with row stride ld inside a buffer of sentinels: a band before, a band after, the slack columns."""

    def __init__(self, rows, cols, dtype, ld):
        self.cols = cols
        self.buf = torch.full((2 * BAND + rows * ld,), SENT, device="cuda", dtype=dtype)
        self.body = self.buf[BAND:BAND + rows * ld].view(rows, ld)
        self.t = self.body[:, :cols]

    def check(self, tag):
        ok = (self.buf[:BAND] == SENT).all() and (self.buf[-BAND:] == SENT).all() and (self.body[:, self.cols:] == SENT).all()
        assert ok, tag + ": guard band or slack columns overwritten"


def _p(t):
    return None if t is None else t.data_ptr()


def bf16_call(lib, tag, x, w, ldw, M, N, K, xmode, res=None, ln_w=None, out_dtype=BF16):
    """vq3_skinny_gemm_bf16 into a guarded [M, N] output with ldy = N + 8. -> the output view (guards checked)."""
    from vggt_qwen3_amd._lib import check
    g = Guard(M, N, out_dtype, N + 8)
    check(lib.vq3_skinny_gemm_bf16(x.data_ptr(), w.data_ptr(), g.t.data_ptr(), _p(res), _p(ln_w), EPS, xmode, M, N, K, x.stride(0), ldw,
                                   N + 8, N, int(out_dtype == F32), stream()), "vq3_skinny_gemm_bf16")
    g.check(tag)
    return g.t


def fp8_call(lib, tag, x, wq, ws, M, N, K, xmode, res=None, ln_w=None):
    """vq3_skinny_gemm_fp8 into a guarded [M, N] bf16 output with ldy = N + 8. -> the output view (guards checked)."""
    from vggt_qwen3_amd._lib import check
    g = Guard(M, N, BF16, N + 8)
    check(lib.vq3_skinny_gemm_fp8(x.data_ptr(), wq.data_ptr(), ws.data_ptr(), g.t.data_ptr(), _p(res), _p(ln_w), EPS, xmode, M, N, K,
                                  x.stride(0), K, N + 8, N, stream()), "vq3_skinny_gemm_fp8")
    g.check(tag)
    return g.t


def bound_bf16(K, ref, sabs, res, out_dtype):
    """Elementwise bound on |y - exact| for y = x W^T (+ res), xmode 0, from the number formats alone.

    A bf16 x bf16 product is exact in fp32 (16 significant bits). The K products are summed in fp32 in some order, every add (the FMA
    chains, the wave reduction, the K-slice combine) rounding once: by the standard summation bound the error is at most
    (K - 1) u / (1 - (K - 1) u) * sum |w| |x| with u = 2^-24, which K * u * sum |w| |x| covers for K <= 10248. Every later rounding adds
    half an ulp of the value it rounds, at most u_b = 2^-8 of it for bf16 (8 significant bits) and u for fp32, and that value is within
    the error so far of the exact one: the bf16 rounding of the product before a residual add, the fp32 add of the residual, and the
    bf16 rounding of a bf16 output."""
    u, ub = 2.0 ** -24, 2.0 ** -8
    e = K * u * sabs
    exact = ref
    if res is not None:
        e = e + ub * (exact.abs() + e)            # the product is a bf16 tensor before the residual add
        exact = ref + res.double()
        e = e + u * (exact.abs() + e)             # the add itself, in fp32
    if out_dtype == BF16:
        e = e + ub * (exact.abs() + e)
    return exact, e + 1e-38                       # below the normal range half an ulp is absolute


def check_bf16_case(ops, lib, data, M, N, K, nmax):
    """One (M, N, K): xmode 0 against fp64, xmode 1 and 2 bit-equal to the stand-alone kernels feeding xmode 0; residual x output type."""
    ref, sabs = data.ref(K, nmax)
    ref, sabs = ref[:M, :N], sabs[:M, :N]
    w, lnw = data.W, data.lnw[:K]
    x = data.x[:M, :K].contiguous()
    gu = data.gu[:M, :2 * K].contiguous()
    xn, xs = ops.rmsnorm_fwd(x, lnw, EPS), ops.silu_mul_fwd(gu)
    worst = 0.0
    for res in (None, data.res[:M, :N].contiguous()):
        for od in (BF16, F32):
            tag = f"skinny bf16 M={M} N={N} K={K} res={res is not None} out={od}"
            y = bf16_call(lib, tag, x, w, KMAX, M, N, K, 0, res, None, od)
            exact, bound = bound_bf16(K, ref, sabs, res, od)
            ratio = ((y.double() - exact).abs() / bound).max().item()
            worst = max(worst, ratio)
            assert ratio <= 1.0, f"{tag}: error is {ratio:.3f} of the bound"
            y1 = bf16_call(lib, tag + " xmode 1", x, w, KMAX, M, N, K, 1, res, lnw, od)
            assert torch.equal(y1, bf16_call(lib, tag, xn, w, KMAX, M, N, K, 0, res, None, od)), tag + ": fused RMSNorm differs"
            y2 = bf16_call(lib, tag + " xmode 2", gu, w, KMAX, M, N, K, 2, res, None, od)
            assert torch.equal(y2, bf16_call(lib, tag, xs, w, KMAX, M, N, K, 0, res, None, od)), tag + ": fused SwiGLU differs"
    return worst


@pytest.mark.parametrize("K", list(BF16_CASES))
def test_bf16_rows_1_2(ops, lib, data, K):
    ns = BF16_CASES[K]
    for N in ns:
        for M in (1, 2):
            print(f"TOL skinny bf16 M={M} N={N} K={K}: worst error / bound {check_bf16_case(ops, lib, data, M, N, K, max(ns)):.3f}")


def test_bf16_rows_3_to_8(ops, lib, data):
    for N in (37, 1030):
        for M in (3, 4, 5, 8):
            print(f"TOL skinny bf16 M={M} N={N} K=520: worst error / bound {check_bf16_case(ops, lib, data, M, N, 520, max(BF16_CASES[520])):.3f}")


def test_bf16_wrapper_equals_c_entry(ops, lib, data):
    """ops.skinny_linear (contiguous weight, its own output) gives the bits of the C entry on a strided weight and a guarded output."""
    M, N, K = 2, 37, 3080
    x, r = data.x[:M, :K].contiguous(), data.res[:M, :N].contiguous()
    y = bf16_call(lib, "wrapper", x, data.W, KMAX, M, N, K, 0, r)
    assert torch.equal(ops.skinny_linear(x, data.W[:N, :K].contiguous(), residual=r), y)


@pytest.mark.parametrize("K", FP8_K)
def test_fp8(ops, lib, data, K):
    Kp = (K + 127) // 128 * 128

    def padded(t, dtype):
        out = torch.zeros((t.shape[0], Kp), device="cuda", dtype=dtype)
        out[:, :K] = t
        return out

    def rel(a, b):
        return ((a.float() - b.float()).norm() / b.float().norm()).item()

    lnw = data.lnw[:K]
    for N in FP8_N:
        wq, ws = ops.quant_fp8_rows(data.W8[:N, :K].contiguous())
        wqp = padded(wq, torch.uint8)
        for M in (1, 2):
            x = data.x[:M, :K].contiguous()
            gu = data.gu[:M, :2 * K].contiguous()
            prepared = (x, ops.rmsnorm_fwd(x, lnw, EPS), ops.silu_mul_fwd(gu))
            for res in (None, data.res[:M, :N].contiguous()):
                for xmode, xin in enumerate((x, x, gu)):
                    tag = f"skinny fp8 M={M} N={N} K={K} xmode={xmode} res={res is not None}"
                    y = fp8_call(lib, tag, xin, wq, ws, M, N, K, xmode, res, lnw if xmode == 1 else None)
                    want = ops.linear_fp8(padded(prepared[xmode], BF16), wqp, ws, residual=res)
                    err = rel(y, want)
                    print(f"TOL {tag}: relative Frobenius error {err:.2e}")
                    assert err < 3e-3, f"{tag}: relative Frobenius error {err:.2e}"
                    yw = ops.skinny_linear_fp8(xin, wq, ws, residual=res, ln_w=lnw if xmode == 1 else None, eps=EPS, swiglu=xmode == 2)
                    assert torch.equal(yw, y), tag + ": wrapper and C entry must give the same bits"


def test_argument_errors(ops, lib):
    from vggt_qwen3_amd._lib import Vq3Error, check
    z = torch.zeros(8 * 256 + 8, device="cuda", dtype=BF16)
    zq, one = torch.zeros(8 * 256 + 16, device="cuda", dtype=torch.uint8), torch.ones(8, device="cuda")
    y = torch.empty(9 * 8, device="cuda", dtype=BF16)

    def bf(M=1, N=8, K=64, xmode=0, ln_w=None, x=z, w=z, ldx=256, ldw=256):
        check(lib.vq3_skinny_gemm_bf16(_p(x), _p(w), y.data_ptr(), None, _p(ln_w), EPS, xmode, M, N, K, ldx, ldw, N, N, 0, stream()), "bf16")

    def f8(M=1, N=8, K=64, xmode=0, ln_w=None, x=z, w=zq, ldx=256, ldw=256):
        check(lib.vq3_skinny_gemm_fp8(_p(x), _p(w), one.data_ptr(), y.data_ptr(), None, _p(ln_w), EPS, xmode, M, N, K, ldx, ldw, N, N,
                                      stream()), "fp8")

    bf(); f8()                                              # the defaults are valid
    with pytest.raises(Vq3Error, match=r"M must be in \[1, 8\]"):
        bf(M=9)
    with pytest.raises(Vq3Error, match="M must be 1 or 2"):
        f8(M=3)
    with pytest.raises(Vq3Error, match=r"skinny_gemm: need N > 0 and K % 8 == 0 \(N=8 K=68\)"):
        bf(K=68)
    with pytest.raises(Vq3Error, match=r"skinny_gemm_fp8: need K % 16 == 0 and K <= 12288 \(N=8 K=72\)"):
        f8(K=72)
    with pytest.raises(Vq3Error, match=r"skinny_gemm_fp8: need K % 16 == 0 and K <= 12288 \(N=8 K=12304\)"):
        f8(K=12304, ldx=12304, ldw=12304)
    with pytest.raises(Vq3Error, match=r"skinny_gemm: xmode must be 0, 1 \(needs ln_w\) or 2"):
        bf(xmode=1)
    with pytest.raises(Vq3Error, match=r"skinny_gemm_fp8: xmode must be 0, 1 \(needs ln_w\) or 2"):
        f8(xmode=1)
    with pytest.raises(Vq3Error, match="skinny_gemm: xmode must be"):
        bf(xmode=3)
    with pytest.raises(Vq3Error, match="skinny_gemm: row strides must cover the row and be multiples of 8"):
        bf(ldx=260)
    with pytest.raises(Vq3Error, match="skinny_gemm_fp8: row strides must cover the row"):
        f8(xmode=2, ldx=64)
    for bad in (dict(x=z[4:]), dict(w=z[4:]), dict(xmode=1, ln_w=z[4:])):
        with pytest.raises(Vq3Error, match="skinny_gemm: operands must be 16-byte aligned"):
            bf(**bad)
    for bad in (dict(x=z[4:]), dict(w=zq[8:]), dict(xmode=1, ln_w=z[4:])):
        with pytest.raises(Vq3Error, match="skinny_gemm_fp8: operands must be 16-byte aligned"):
            f8(**bad)
