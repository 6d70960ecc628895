"""The decode GEMM for 1..64 rows (decode_gemm.hip: vq3_decode_gemm_bf16) on every instantiation and every K-split branch the dispatcher
can reach, at the smallest shapes that select them.

Dispatch (decode_gemm.hip: plan_decode). A workgroup owns 64 weight rows and one K slice. The kernel is instantiated per
(MT = ceil(M / 16) in 1..4, xmode in 0..2): 12 kernels. KS, the number of K slices, is a grid dimension: doubled from 1 while
ceil(N / 64) * KS < 256, 2 * KS <= ceil(K / 256) and KS < 8. With KS > 1 the slices meet in the workspace and a second kernel
(one instantiation per MT) adds them in slice order and runs the epilogue.

Case -> what it reaches. Every case runs M = 1, 9, 16, 17, 32, 33, 48, 64 (MT 1, 1, 1, 2, 2, 3, 3, 4: every MT with a full and a partly
used last tile), xmode 0, 1 and 2, with and without a residual, bf16 and fp32 output:
  K 520    3 chunks of 256, the last one 8 elements:   N 37, 1030 -> KS 2 (slices of 2 and 1 chunks);  N 16321 -> KS 1
  K 3080   13 chunks, the last one 8 elements:         N 37, 1030 -> KS 8 (2 chunks per slice: slice 6 has one, slice 7 none);
                                                       N 4033 -> KS 4;  N 8129 -> KS 2;  N 16321 -> KS 1
  K 10248  41 chunks, the last one 8 elements:         N 37, 1030 -> KS 8 (6 chunks per slice, slice 7 none);  N 16321 -> KS 1
4033, 8129 and 16321 are the smallest N with 64, 128 and 256 workgroups per slice. None of the K is a multiple of 32 (the MFMA's k), of
64 (a K block) or of 256 (a chunk): the clamped weight loads and the zeroed x past K. None of the N is a multiple of 64 (rows per
workgroup) or of 16 (rows per wave): N 37 leaves one wave of the workgroup without any row.

What is asserted.
  test_exact_integers   x and W hold integers in [-4, 4]: |sum| <= 16 * 10248 < 2^24, so every partial sum is exact in any order and
                        the fp32 output must equal the fp64 product bit for bit; bf16 output and the residual variants must equal
                        torch's roundings of it. Catches every fragment, tail, slice and slack-row indexing error with no tolerance.
  test_random_vs_fp64   xmode 0 against the fp64 product of the bf16 operands, with bound_bf16() of tests/test_skinny_gemm_gpu.py
                        restated here and C = 1: that derivation lets every fp32 add round once, which is not documented for the
                        MFMA's internal adder, so C is the place where a measured allowance for it would go (see C below). xmode 1
                        and 2 must be bit-equal to ops.rmsnorm_fwd / ops.silu_mul_fwd feeding xmode 0 of the same entry. Two calls
                        with the same arguments must give the same bits (every KS).
  test_dispatch_and_argument_errors
Every output is written through the C entry into a buffer with sentinel bands before and after and sentinel slack columns
(ldy = N + 8) that must come back unchanged; the weight is a strided view (ldw = 10248 > K); the K-slice workspace is handed over
filled with 0xAB bytes (the entry must not rely on its contents). `pytest -s` prints the worst error / bound ratio per case."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EPS = 1e-6
SENT = 777.0
BAND = 4096
KMAX, NMAX, MMAX = 10248, 16321, 64
MS = (1, 9, 16, 17, 32, 33, 48, 64)
CASES = {520: (37, 1030, 16321), 3080: (37, 1030, 4033, 8129, 16321), 10248: (37, 1030, 16321)}
# (K, N) -> KS, as listed in the module docstring (checked against the library's workspace size)
KS = {(520, 37): 2, (520, 1030): 2, (520, 16321): 1, (3080, 37): 8, (3080, 1030): 8, (3080, 4033): 4, (3080, 8129): 2, (3080, 16321): 1,
      (10248, 37): 8, (10248, 1030): 8, (10248, 16321): 1}
C = 1.0     # factor on the fp32 summation term of bound_bf16: 1 holds (worst measured error / bound 0.944 over all cases)


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


def ints(shape, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(-4, 5, shape, generator=g, device="cuda").to(BF16)


class Data:
    """Operands created once per module; every case reads a leading block of them. The fp64 references are computed once per K."""

    def __init__(self):
        self.W = rnd((NMAX, KMAX), 1, 0.05)                       # 334 MB; a case's weight is W[:N, :K] with ldw = KMAX
        self.x = rnd((MMAX, KMAX), 2)
        self.gu = rnd((MMAX, 2 * KMAX), 3)
        self.lnw = (1 + rnd((KMAX,), 4, 0.2, F32)).to(BF16)
        self.res = rnd((MMAX, NMAX), 5)
        self.Wi = ints((NMAX, KMAX), 6)
        self.xi = ints((MMAX, KMAX), 7)
        self._ref, self._iref = {}, {}

    def ref(self, K):
        """(x W^T, |x| |W|^T) in fp64 for the 64 rows of x[:, :K] and the rows of W[:, :K] the K's cases use."""
        if K not in self._ref:
            x, w = self.x[:, :K].double(), self.W[:max(CASES[K]), :K].double()
            self._ref[K] = (x @ w.t(), x.abs() @ w.abs().t())
        return self._ref[K]

    def iref(self, K):
        if K not in self._iref:
            self._iref[K] = self.xi[:, :K].double() @ self.Wi[:max(CASES[K]), :K].double().t()
        return self._iref[K]


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


def call(lib, tag, x, w, ldw, M, N, K, xmode, res=None, ln_w=None, out_dtype=BF16):
    """vq3_decode_gemm_bf16 into a guarded [M, N] output with ldy = N + 8. -> the output view (guards checked)."""
    from vggt_qwen3_amd._lib import check
    g = Guard(M, N, out_dtype, N + 8)
    nbytes = int(lib.vq3_decode_gemm_workspace_bytes(M, N, K))
    ws = torch.full((nbytes,), 0xAB, device="cuda", dtype=torch.uint8) if nbytes else None
    check(lib.vq3_decode_gemm_bf16(x.data_ptr(), w.data_ptr(), g.t.data_ptr(), _p(res), _p(ln_w), EPS, xmode, M, N, K, x.stride(0), ldw,
                                   N + 8, N, int(out_dtype == F32), _p(ws), nbytes, stream()), "vq3_decode_gemm_bf16")
    g.check(tag)
    return g.t


def bound_bf16(K, ref, sabs, res, out_dtype):
    """Elementwise bound on |y - exact| for y = x W^T (+ res), xmode 0, from the number formats alone (test_skinny_gemm_gpu.py).

    A bf16 x bf16 product is exact in fp32 (16 significant bits). The K products are summed in fp32 in some order, every add (inside
    the MFMA, across MFMAs, the K-slice combine) rounding once: by the standard summation bound the error is at most
    (K - 1) u / (1 - (K - 1) u) * sum |w| |x| with u = 2^-24, which K * u * sum |w| |x| covers for K <= 10248; C scales this term. Every
    later rounding adds half an ulp of the value it rounds, at most u_b = 2^-8 of it for bf16 (8 significant bits) and u for fp32, and
    that value is within the error so far of the exact one: the bf16 rounding of the product before a residual add, the fp32 add of
    the residual, and the bf16 rounding of a bf16 output."""
    u, ub = 2.0 ** -24, 2.0 ** -8
    e = C * K * u * sabs
    exact = ref
    if res is not None:
        e = e + ub * (exact.abs() + e)            # the product is a bf16 tensor before the residual add
        exact = ref + res.double()
        e = e + u * (exact.abs() + e)             # the add itself, in fp32
    if out_dtype == BF16:
        e = e + ub * (exact.abs() + e)
    return exact, e + 1e-38                       # below the normal range half an ulp is absolute


def workspace_slices(lib, M, N, K):
    """KS as the library's workspace size tells it: KS fp32 tiles of 64 weight rows x 16 MT batch rows per workgroup (0: KS = 1)."""
    nbytes = int(lib.vq3_decode_gemm_workspace_bytes(M, N, K))
    if nbytes == 0:
        return 1
    groups, mt = (N + 63) // 64, (M + 15) // 16
    assert nbytes % (groups * 4 * mt * 256 * 4) == 0
    return nbytes // (groups * 4 * mt * 256 * 4)


@pytest.mark.parametrize("K", list(CASES))
def test_exact_integers(lib, data, K):
    for N in CASES[K]:
        exact = data.iref(K)
        for M in MS:
            assert workspace_slices(lib, M, N, K) == KS[K, N], (M, N, K)
            x, res, want = data.xi[:M, :K].contiguous(), data.res[:M, :N].contiguous(), exact[:M, :N]
            tag = f"decode gemm integers M={M} N={N} K={K}"
            assert torch.equal(call(lib, tag, x, data.Wi, KMAX, M, N, K, 0, None, None, F32).double(), want), tag + ": fp32 output"
            prod = want.float().to(BF16)
            assert torch.equal(call(lib, tag, x, data.Wi, KMAX, M, N, K, 0, None, None, BF16), prod), tag + ": bf16 output"
            summed = prod.float() + res.float()
            assert torch.equal(call(lib, tag, x, data.Wi, KMAX, M, N, K, 0, res, None, F32), summed), tag + ": residual, fp32 output"
            assert torch.equal(call(lib, tag, x, data.Wi, KMAX, M, N, K, 0, res, None, BF16), summed.to(BF16)), tag + ": residual, bf16 output"


def check_random_case(ops, lib, data, M, N, K):
    """One (M, N, K): xmode 0 against fp64, xmode 1 and 2 bit-equal to the stand-alone kernels feeding xmode 0; residual x output type."""
    ref, sabs = data.ref(K)
    ref, sabs = ref[:M, :N], sabs[:M, :N]
    w, lnw = data.W, data.lnw[:K]
    x = data.x[:M, :K].contiguous()
    gu = data.gu[:M, :2 * K].contiguous()
    xn, xs = ops.rmsnorm_fwd(x, lnw, EPS), ops.silu_mul_fwd(gu)
    worst = 0.0
    for res in (None, data.res[:M, :N].contiguous()):
        for od in (BF16, F32):
            tag = f"decode gemm M={M} N={N} K={K} res={res is not None} out={od}"
            y = call(lib, tag, x, w, KMAX, M, N, K, 0, res, None, od)
            exact, bound = bound_bf16(K, ref, sabs, res, od)
            ratio = ((y.double() - exact).abs() / bound).max().item()
            worst = max(worst, ratio)
            assert ratio <= 1.0, f"{tag}: error is {ratio:.3f} of the bound"
            assert torch.equal(y, call(lib, tag, x, w, KMAX, M, N, K, 0, res, None, od)), tag + ": two calls differ"
            y1 = call(lib, tag + " xmode 1", x, w, KMAX, M, N, K, 1, res, lnw, od)
            assert torch.equal(y1, call(lib, tag, xn, w, KMAX, M, N, K, 0, res, None, od)), tag + ": fused RMSNorm differs"
            y2 = call(lib, tag + " xmode 2", gu, w, KMAX, M, N, K, 2, res, None, od)
            assert torch.equal(y2, call(lib, tag, xs, w, KMAX, M, N, K, 0, res, None, od)), tag + ": fused SwiGLU differs"
    return worst


@pytest.mark.parametrize("K", list(CASES))
def test_random_vs_fp64(ops, lib, data, K):
    for N in CASES[K]:
        for M in MS:
            print(f"TOL decode gemm M={M} N={N} K={K} KS={KS[K, N]}: worst error / bound {check_random_case(ops, lib, data, M, N, K):.3f}")


def test_dispatch_and_argument_errors(ops, lib, data):
    from vggt_qwen3_amd._lib import Vq3Error, check
    # the wrapper: up to 8 rows it IS skinny_linear, above it gives the bits of the C entry on a strided weight and a guarded output
    N, K = 1030, 3080
    w = data.W[:N, :K].contiguous()
    x8, r8 = data.x[:8, :K].contiguous(), data.res[:8, :N].contiguous()
    for kw in (dict(), dict(residual=r8), dict(ln_w=data.lnw[:K], eps=EPS), dict(out_dtype=F32)):
        assert torch.equal(ops.decode_linear(x8, w, **kw), ops.skinny_linear(x8, w, **kw))
    gu8 = data.gu[:8, :2 * K].contiguous()
    assert torch.equal(ops.decode_linear(gu8, w, swiglu=True), ops.skinny_linear(gu8, w, swiglu=True))
    x9, r9 = data.x[:9, :K].contiguous(), data.res[:9, :N].contiguous()
    assert torch.equal(ops.decode_linear(x9, w, residual=r9), call(lib, "wrapper", x9, data.W, KMAX, 9, N, K, 0, r9))
    assert torch.equal(ops.decode_linear(x9, w, n=N - 3), ops.decode_linear(x9, w)[:, :N - 3])
    assert ops.DECODE_MAX_ROWS == 64
    with pytest.raises(Vq3Error, match=r"M must be in \[1, 8\]"):
        ops.skinny_linear(x9, w)
    with pytest.raises(ValueError, match="at most 64 rows"):
        ops.decode_linear(torch.zeros(65, K, device="cuda", dtype=BF16), w)

    z = torch.zeros(64 * 256 + 8, device="cuda", dtype=BF16)
    y = torch.empty(65 * 8, device="cuda", dtype=BF16)
    ws = torch.zeros(1 << 20, device="cuda", dtype=torch.uint8)

    def dg(M=1, N=8, K=64, xmode=0, ln_w=None, x=z, w=z, ldx=256, ldw=256, ws=ws, nws=1 << 20):
        check(lib.vq3_decode_gemm_bf16(_p(x), _p(w), y.data_ptr(), None, _p(ln_w), EPS, xmode, M, N, K, ldx, ldw, N, N, 0, _p(ws), nws,
                                       stream()), "decode_gemm")

    dg(); dg(M=64)                                          # the defaults are valid
    for M in (0, 65):
        with pytest.raises(Vq3Error, match=rf"decode_gemm: M must be in \[1, 64\], got {M}"):
            dg(M=M)
    with pytest.raises(Vq3Error, match=r"decode_gemm: need N > 0 and K % 8 == 0 \(N=8 K=68\)"):
        dg(K=68)
    with pytest.raises(Vq3Error, match=r"decode_gemm: xmode must be 0, 1 \(needs ln_w\) or 2"):
        dg(xmode=1)
    with pytest.raises(Vq3Error, match="decode_gemm: xmode must be"):
        dg(xmode=3)
    with pytest.raises(Vq3Error, match="decode_gemm: row strides must cover the row and be multiples of 8"):
        dg(ldx=260)
    with pytest.raises(Vq3Error, match="decode_gemm: row strides must cover the row"):
        dg(xmode=2, ldx=64)
    for bad in (dict(x=z[4:]), dict(w=z[4:]), dict(xmode=1, ln_w=z[4:])):
        with pytest.raises(Vq3Error, match="decode_gemm: operands must be 16-byte aligned"):
            dg(**bad)
    # K = 512 at N = 8 is cut into 2 slices: the workspace is required, and large enough
    need = int(lib.vq3_decode_gemm_workspace_bytes(64, 8, 512))
    assert need > 0 and int(lib.vq3_decode_gemm_workspace_bytes(64, 8, 256)) == 0
    big = torch.zeros(64 * 512, device="cuda", dtype=BF16)
    dg(M=64, K=512, x=big, w=big, ldx=512, ldw=512)
    dg(M=64, K=256, ws=None, nws=0)                        # no slices, no workspace
    for kw in (dict(ws=None, nws=0), dict(nws=need - 1)):
        with pytest.raises(Vq3Error, match=rf"decode_gemm: M=64 N=8 K=512 is cut into 2 K slices and needs {need} bytes"):
            dg(M=64, K=512, x=big, w=big, ldx=512, ldw=512, **kw)
