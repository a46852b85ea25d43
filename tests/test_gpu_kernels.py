"""Single-launch parity of the encoder kernels against numpy float64 (tests/native/kernel_harness.hip drives one launcher of
csrc/kernels.h per call from host buffers with guard bands and poisoned outputs).  Every case is labelled with the kernel the launcher is
meant to pick (kernel_harness.gemm_path / layernorm_path, a restatement of the launchers' predicates), and every reference is computed
from the exact f16 / f32 operands the kernel received.

Bounds (u = 2^-24, the fp32 unit roundoff; C = 2 throughout):
  * fp32 GEMM outputs: |got - ref| <= C u (K_eff |A| |W|^T + |bias| + |added|), K_eff = K (2 K for a split A operand: hi and lo products
    accumulate into the same fp32 sum), `added` the positional row (CONV2) or the initial residual (RESID_F32) - a sum of K_eff exact
    f16 products and one more term per addend, each rounding at most u times the magnitude it touches;
  * f16 outputs: that bound plus half an f16 ulp of the reference; split outputs check hi + lo at the split's own precision (2^-22
    relative, 2^-25 absolute below the f16 normal range) instead;
  * GELU outputs: the pre-activation bound times max |GELU'| (1.13) plus twice the error of gelu_erf_fast measured on the CPU
    (tests/test_kernel_harness.py);
  * CROSS_KV: hi + lo * hr24_unit(hi) within hr24_unit(hi) (the encoder's rounding, and the clamp at |r| = 128) plus the fp32 bound.
"""
import numpy as np
import pytest

import kernel_harness as KH
from kernel_harness import (CTX, CTX_PAD, EPI_CONV1, EPI_CONV2, EPI_CROSS_KV, EPI_F16, EPI_F32, EPI_GELU_F16, EPI_QKV_ENC,
                            EPI_RESID_F32, FRAMES, FRAMES_PAD)
from whisperkit_amd import weights

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C_BOUND = 2.0
GELU_SLOPE = 1.13          # max |d/dx x Phi(x)| = 1.1289 (at x = sqrt 2)
GELU_FAST_ERR = 2.0 * KH.GELU_FAST_ERR_MEASURED   # 2 x the max |gelu_erf_fast - gelu| / max(1, |x|) measured on the CPU (test_kernel_harness.py)
F16_NAN = np.uint16(0x7E00)


@pytest.fixture(scope="module")
def kh(tmp_path_factory):
    return KH.Harness(KH.build(tmp_path_factory.mktemp("kernel_harness")))


def ok(res):
    status, guard = res
    assert status == 0, f"HIP status {status}"
    assert guard == 0, f"{guard} guard bytes changed (a write outside the allocation)"


def poison16(shape):
    return np.full(shape, F16_NAN, np.uint16).view(np.float16)


def poison32(shape):
    return np.full(shape, np.nan, np.float32)


def operands(rng, rows, cols, mean=0.25, scale=1.0):
    """f16 operand with a nonzero mean (a dropped term does not cancel out)"""
    return (mean + scale * rng.standard_normal((rows, cols))).astype(np.float16)


def is_poison16(x):
    return x.view(np.uint16) == F16_NAN


def check_f16(got, ref, bound32, what):
    assert not is_poison16(got).any(), f"{what}: {int(is_poison16(got).sum())} elements never written"
    err = np.abs(got.astype(np.float64) - ref)
    lim = bound32 + KH.f16_half_ulp(np.abs(ref) + bound32)
    bad = err > lim
    assert not bad.any(), f"{what}: {int(bad.sum())} elements out of bound, worst excess {float((err - lim).max()):.3e}"


def check_f32(got, ref, bound32, what):
    assert not np.isnan(got).any(), f"{what}: {int(np.isnan(got).sum())} elements never written"
    err = np.abs(got.astype(np.float64) - ref)
    bad = err > bound32
    assert not bad.any(), f"{what}: {int(bad.sum())} elements out of bound, worst excess {float((err - bound32).max()):.3e}"


def check_split(hi, lo, ref, bound32, what):
    assert not is_poison16(hi).any() and not is_poison16(lo).any(), f"{what}: lo / hi elements never written"
    got = hi.astype(np.float64) + lo.astype(np.float64)
    lim = bound32 + np.maximum(np.abs(ref) * 2.0 ** -22, 2.0 ** -25)
    err = np.abs(got - ref)
    assert (err <= lim).all(), f"{what}: {int((err > lim).sum())} elements out of bound, worst excess {float((err - lim).max()):.3e}"


# ---------------------------------------------------------------------------------------------- GEMM
class Gemm:
    """One launch_gemm case: operands, the overlapping-row view of the A rows, fp64 reference and its bound"""

    def __init__(self, epi, M, N, K, seed, lda=None, a_rows=None, a_stride=0, a_buf=None, split=False, d=0, bias_scale=0.5):
        rng = np.random.default_rng(seed)
        self.epi, self.M, self.N, self.K, self.split, self.d = epi, M, N, K, split, d
        self.lda = K if lda is None else lda
        self.a_rows = M if a_rows is None else a_rows
        self.a_stride = a_stride
        if a_buf is None:
            a_buf = operands(rng, M, self.lda)
        self.A = a_buf
        # the split form's lo plane: f16(x - f16(x)) of an fp32 operand whose hi plane is A
        self.A_lo = (rng.uniform(-1, 1, a_buf.shape) * np.abs(a_buf.astype(np.float32)) * 2.0 ** -11).astype(np.float16) if split else None
        self.W = (0.1 + 0.3 * rng.standard_normal((N, K)) / np.sqrt(K / 64)).astype(np.float16)
        self.bias = (bias_scale * rng.standard_normal(N) + 0.1).astype(np.float32)
        self.rng = rng

    def rows(self, buf):
        """the logical [M][K] operand: address(m, k) = (m / a_rows) * a_stride + (m % a_rows) * lda + k"""
        flat = buf.reshape(-1)
        m = np.arange(self.M)
        start = (m // self.a_rows) * self.a_stride + (m % self.a_rows) * self.lda
        return flat[start[:, None] + np.arange(self.K)[None, :]]

    def reference(self):
        A = self.rows(self.A).astype(np.float64)
        absA = np.abs(A)
        kk = self.K
        if self.split:
            Alo = self.rows(self.A_lo).astype(np.float64)
            absA = absA + np.abs(Alo)
            A = A + Alo
            kk = 2 * self.K
        W = self.W.astype(np.float64)
        ref = A @ W.T + self.bias.astype(np.float64)
        bound = C_BOUND * U * (kk * (absA @ np.abs(W).T) + np.abs(self.bias.astype(np.float64)))
        return ref, bound

    def launch(self, kh, arrays, ldc, offsets=None, rows_per_batch_out=0, max_batch=0):
        arrays = dict(arrays, A=self.A, A_lo=self.A_lo, W=self.W, bias=self.bias)
        return kh.gemm(self.epi, self.M, self.N, self.K, self.lda, ldc, arrays, a_rows_per_batch=self.a_rows, a_batch_stride=self.a_stride,
                       d_model=self.d, rows_per_batch_out=rows_per_batch_out, max_batch=max_batch, offsets=offsets)

    def path(self, ldc, out_align=16):
        return KH.gemm_path(self.M, self.N, self.K, self.lda, self.a_stride, ldc, self.d, self.epi, self.split, out_align)


def run_rowmajor(kh, g, ldc=None, out_off=0, expect=None):
    """EPI_F16 / GELU_F16 / F32 / RESID_F32 into an [M][ldc] output (columns N .. ldc - 1 must stay poisoned)"""
    ldc = g.N if ldc is None else ldc
    path = g.path(ldc, 16 if out_off % 16 == 0 else 8)
    if expect is not None:
        assert path.startswith(expect), (path, expect)
    ref, bound = g.reference()
    arrays = {}
    split_lo = g.split and g.epi == EPI_GELU_F16
    if g.epi in (EPI_F32, EPI_RESID_F32):
        out = poison32((g.M, ldc))
        if g.epi == EPI_RESID_F32:
            init = (0.5 + g.rng.standard_normal((g.M, ldc))).astype(np.float32)
            out[:] = init
            out[:, g.N:] = np.nan
            ref = ref + init[:, :g.N].astype(np.float64)
            bound = bound + C_BOUND * U * np.abs(init[:, :g.N].astype(np.float64))
        arrays["out32"] = out
        ok(g.launch(kh, arrays, ldc, offsets={"out32": out_off}))
        check_f32(out[:, :g.N], ref, bound, path)
        assert np.isnan(out[:, g.N:]).all(), f"{path}: write into the ldc padding"
        return path
    out = poison16((g.M, ldc))
    arrays["out16"] = out
    lo = None
    if split_lo:
        lo = poison16((g.M, ldc))
        arrays["out16_lo"] = lo
    ok(g.launch(kh, arrays, ldc, offsets={"out16": out_off, "out16_lo": out_off}))
    if g.epi == EPI_GELU_F16:
        bound = GELU_SLOPE * bound + GELU_FAST_ERR * np.maximum(1.0, np.abs(ref))
        ref = KH.gelu_f64(ref)
    if split_lo:
        check_split(out[:, :g.N], lo[:, :g.N], ref, bound, path)
        assert is_poison16(lo[:, g.N:]).all(), f"{path}: write into the ldc padding of the lo plane"
    else:
        check_f16(out[:, :g.N], ref, bound, path)
    assert is_poison16(out[:, g.N:]).all(), f"{path}: write into the ldc padding"
    return path


# (epi, M, N, K, ldc, out offset, split, expected kernel): each path one step on either side of its tile-count threshold, M tails
# (M % 256 in {4, 220, 252}), N = 3 d / 4 d at d = 384 (not a multiple of 256), K = 240 (not a multiple of 32) and 384
ROWMAJOR_CASES = [
    (EPI_F16, 500, 384, 384, 392, 0, False, "gemm_kernel<64,64>"),          # tiles128 = 16
    (EPI_F16, 2004, 1536, 240, 1536, 0, False, "gemm_kernel<128,128>"),     # tiles128 = 16 x 12 = 192, K % 64 != 0
    (EPI_F16, 1900, 1536, 384, 1536, 0, False, "gemm_kernel<64,64>"),       # tiles128 = 15 x 12 = 180 < 192 (tiles256 = 48)
    (EPI_GELU_F16, 4100, 1152, 384, 1152, 0, False, "gemm256_kernel<mode 1>"),   # tiles256 = 17 x 5 = 85
    (EPI_GELU_F16, 3804, 1024, 384, 1024, 0, False, "gemm_kernel<128,128>"),     # tiles256 = 15 x 4 = 60 < 64, tiles128 = 30 x 8 = 240
    (EPI_F16, 4004, 1024, 384, 1024, 0, False, "gemm256_kernel<mode 1>"),   # tiles256 = 16 x 4 = 64
    (EPI_F16, 4004, 1024, 384, 1024, 8, False, "gemm256_kernel<mode 0>"),   # 8-byte output offset: the direct epilogue
    (EPI_F16, 4004, 1000, 384, 1000, 0, False, "gemm256_kernel<mode 0>"),   # N % 64 != 0
    (EPI_F16, 4002, 1024, 384, 1024, 0, False, "gemm256_kernel<mode 0>"),   # M % 4 != 0
    (EPI_GELU_F16, 4004, 1024, 384, 1024, 8, False, "gemm256_kernel<mode 0>"),
    (EPI_F16, 4004, 1024, 240, 1024, 0, False, "gemm_kernel<128,128>"),     # K % 64 != 0 keeps the 256 tile away
    (EPI_RESID_F32, 3004, 1536, 384, 1544, 0, False, "gemm256_kernel<mode 1>"),  # tiles256 = 12 x 6 = 72, ldc padding
    (EPI_RESID_F32, 3004, 1480, 384, 1480, 0, False, "gemm256_kernel<mode 0>"),  # N % 64 != 0
    (EPI_RESID_F32, 1500, 384, 1536, 384, 0, False, "gemm_kernel<64,64>"),
    (EPI_F32, 3004, 1536, 384, 1536, 0, False, "gemm256_kernel<mode 0>"),   # no staged form for F32
    (EPI_F32, 700, 200, 240, 208, 0, False, "gemm_kernel<64,64>"),
    # split A operand (BK = 32: K = 240 is still not whole tiles, K = 288 is for the split kernels only)
    (EPI_GELU_F16, 4100, 1152, 288, 1152, 0, True, "gemm256_split_kernel<mode 1>"),
    (EPI_GELU_F16, 4004, 1024, 384, 1024, 8, True, "gemm256_split_kernel<mode 0>"),
    (EPI_F16, 3004, 1536, 288, 1536, 0, True, "gemm256_split_kernel<mode 1>"),
    (EPI_RESID_F32, 3004, 1536, 384, 1536, 0, True, "gemm256_split_kernel<mode 1>"),
    (EPI_F32, 3804, 1024, 384, 1024, 0, True, "gemm_split_kernel<128,128>"),
    (EPI_GELU_F16, 2004, 1536, 240, 1536, 0, True, "gemm_split_kernel<128,128>"),
    (EPI_GELU_F16, 1900, 1536, 240, 1536, 0, True, "gemm_split_kernel<64,64>"),
    (EPI_RESID_F32, 500, 384, 384, 384, 0, True, "gemm_split_kernel<64,64>"),
]


@pytest.mark.parametrize("case", ROWMAJOR_CASES, ids=[f"{c[7]}-epi{c[0]}-{c[1]}x{c[2]}x{c[3]}-ldc{c[4]}-off{c[5]}" for c in ROWMAJOR_CASES])
def test_gemm_rowmajor_epilogues_vs_fp64(kh, case):
    epi, M, N, K, ldc, off, split, expect = case
    g = Gemm(epi, M, N, K, seed=M + N + K + epi, split=split)
    run_rowmajor(kh, g, ldc=ldc, out_off=off, expect=expect)


def run_qkv(kh, d, batch, split=False, out_off=0, expect=None, seed=3):
    M, N = batch * CTX, 3 * d
    g = Gemm(EPI_QKV_ENC, M, N, d, seed=seed + d + batch, split=split, d=d)
    path = g.path(d, 16 if out_off % 16 == 0 else 8)
    if expect is not None:
        assert path.startswith(expect), (path, expect)
    q, k, vt = poison16((M, d)), poison16((M, d)), poison16((batch, d, CTX_PAD))
    ok(g.launch(kh, dict(out16=q, k16=k, vt16=vt), d, offsets=dict(out16=out_off, k16=out_off, vt16=out_off), rows_per_batch_out=CTX))
    ref, bound = g.reference()
    check_f16(q, ref[:, :d], bound[:, :d], path + " q")
    check_f16(k, ref[:, d:2 * d], bound[:, d:2 * d], path + " k")
    vref = ref[:, 2 * d:].reshape(batch, CTX, d).transpose(0, 2, 1)
    vbound = bound[:, 2 * d:].reshape(batch, CTX, d).transpose(0, 2, 1)
    check_f16(vt[:, :, :CTX], vref, vbound, path + " V^T")
    assert is_poison16(vt[:, :, CTX:]).all(), f"{path}: write into the V^T pad columns 1500 .. 1535"
    return path


@pytest.mark.parametrize("d,batch,off,expect", [(384, 1, 0, "gemm_kernel<64,64>"), (384, 3, 0, "gemm256_kernel<mode 1>"),
                                                (384, 3, 8, "gemm256_kernel<mode 0>"), (512, 3, 0, "gemm256_kernel<mode 1>"),
                                                (768, 1, 0, "gemm_kernel<128,128>"), (1280, 1, 0, "gemm256_kernel<mode 1>"), (1280, 3, 8, "gemm256_kernel<mode 0>")])
def test_gemm_qkv_enc_layout_vs_fp64(kh, d, batch, off, expect):
    run_qkv(kh, d, batch, out_off=off, expect=expect)


def test_gemm_qkv_enc_split_vs_fp64(kh):
    run_qkv(kh, 768, 3, split=True, expect="gemm256_split_kernel<mode 1>")


def run_conv1(kh, n_mels, d, batch, split=False, expect=None):
    """conv1 (k3 s1 p1) over the padded time-major mel: lda = n_mels, K = 3 n_mels, rows t + 1 of a 3002-row output per batch"""
    rng = np.random.default_rng(n_mels + d + batch)
    mel = operands(rng, batch * FRAMES_PAD, n_mels).reshape(batch, FRAMES_PAD, n_mels)
    mel[:, 0] = 0
    mel[:, FRAMES_PAD - 1] = 0
    g = Gemm(EPI_CONV1, batch * FRAMES, d, 3 * n_mels, seed=5, lda=n_mels, a_rows=FRAMES, a_stride=FRAMES_PAD * n_mels,
             a_buf=np.ascontiguousarray(mel), split=split)
    path = g.path(d)
    if expect is not None:
        assert path.startswith(expect), (path, expect)
    out = poison16((batch, FRAMES_PAD, d))
    arrays = dict(out16=out)
    lo = None
    if split:
        lo = poison16((batch, FRAMES_PAD, d))
        arrays["out16_lo"] = lo
    ok(g.launch(kh, arrays, d, rows_per_batch_out=FRAMES))
    ref, bound = g.reference()
    bound = GELU_SLOPE * bound + GELU_FAST_ERR * np.maximum(1.0, np.abs(ref))
    ref = KH.gelu_f64(ref).reshape(batch, FRAMES, d)
    bound = bound.reshape(batch, FRAMES, d)
    if split:
        check_split(out[:, 1:FRAMES + 1], lo[:, 1:FRAMES + 1], ref, bound, path + " conv1")
        assert is_poison16(lo[:, [0, FRAMES_PAD - 1]]).all()
    else:
        check_f16(out[:, 1:FRAMES + 1], ref, bound, path + " conv1")
    assert is_poison16(out[:, [0, FRAMES_PAD - 1]]).all(), f"{path}: conv1 wrote a zero-padding row (t = 0 / 3001)"
    return path


@pytest.mark.parametrize("n_mels,d,batch,expect", [(80, 384, 1, "gemm_kernel<64,64>"), (80, 1280, 3, "gemm_kernel<128,128>"),
                                                   (128, 1280, 3, "gemm256_kernel<mode 0>"), (128, 512, 1, "gemm_kernel<64,64>")])
def test_gemm_conv1_view_vs_fp64(kh, n_mels, d, batch, expect):
    run_conv1(kh, n_mels, d, batch, expect=expect)


def test_gemm_conv1_split_vs_fp64(kh):
    run_conv1(kh, 128, 1280, 3, split=True, expect="gemm256_split_kernel<mode 0>")


def run_conv2(kh, d, batch, split=False, expect=None):
    """conv2 (k3 s2 p1): lda = 2 d over the 3002-row conv1 output, + positional rows"""
    rng = np.random.default_rng(d + batch + 7)
    h1 = operands(rng, batch * FRAMES_PAD, d).reshape(batch, FRAMES_PAD, d)
    h1[:, 0] = 0
    h1[:, FRAMES_PAD - 1] = 0
    g = Gemm(EPI_CONV2, batch * CTX, d, 3 * d, seed=9, lda=2 * d, a_rows=CTX, a_stride=FRAMES_PAD * d, a_buf=np.ascontiguousarray(h1),
             split=split)
    path = g.path(d)
    if expect is not None:
        assert path.startswith(expect), (path, expect)
    pos = rng.standard_normal((CTX, d)).astype(np.float32)
    out = poison32((batch * CTX, d))
    ok(g.launch(kh, dict(out32=out, pos=pos), d, rows_per_batch_out=CTX))
    ref, bound = g.reference()
    posr = np.tile(pos.astype(np.float64), (batch, 1))
    bound = GELU_SLOPE * bound + GELU_FAST_ERR * np.maximum(1.0, np.abs(ref)) + C_BOUND * U * (np.abs(posr) + np.abs(KH.gelu_f64(ref)))
    check_f32(out, KH.gelu_f64(ref) + posr, bound, path + " conv2")
    return path


@pytest.mark.parametrize("d,batch,expect", [(384, 1, "gemm_kernel<64,64>"), (512, 3, "gemm_kernel<64,64>"),
                                            (768, 3, "gemm_kernel<128,128>"), (1024, 3, "gemm256_kernel<mode 0>")])
def test_gemm_conv2_view_vs_fp64(kh, d, batch, expect):
    run_conv2(kh, d, batch, expect=expect)


def test_gemm_conv2_split_vs_fp64(kh):
    run_conv2(kh, 1024, 3, split=True, expect="gemm256_split_kernel<mode 0>")


def run_cross_kv(kh, d, L, batch, max_batch, A=None, bias=None, split=False, expect=None, seed=13):
    M, N, H = batch * CTX, L * 2 * d, d // 64
    g = Gemm(EPI_CROSS_KV, M, N, d, seed=seed + d, a_buf=A, split=split, d=d)
    if bias is not None:
        g.bias = bias
    path = g.path(N)
    if expect is not None:
        assert path.startswith(expect), (path, expect)
    shape = (L, max_batch, H, CTX, 64)
    khi, vhi = poison16(shape), poison16(shape)
    klo, vlo = np.full(shape, -128, np.int8), np.full(shape, -128, np.int8)
    ok(g.launch(kh, dict(kv_k_hi=khi, kv_v_hi=vhi, kv_k_lo=klo, kv_v_lo=vlo), N, max_batch=max_batch))
    ref, bound = g.reference()
    # n = l * 2d + kv * d + h * 64 + c, m = b * 1500 + t  ->  [l][b][h][t][c]
    r = ref.reshape(batch, CTX, L, 2, H, 64).transpose(3, 2, 0, 4, 1, 5)
    bd = bound.reshape(batch, CTX, L, 2, H, 64).transpose(3, 2, 0, 4, 1, 5)
    for kv, (hi, lo) in enumerate(((khi, klo), (vhi, vlo))):
        h_ = hi[:, :batch]
        assert not is_poison16(h_).any(), f"{path}: cross {'KV'[kv]} rows never written"
        unit = KH.hr24_unit(h_.view(np.uint16))
        got = h_.astype(np.float64) + lo[:, :batch].astype(np.float64) * unit
        err = np.abs(got - r[kv])
        lim = unit + bd[kv]
        assert (err <= lim).all(), f"{path}: cross {'KV'[kv]} {int((err > lim).sum())} out of bound, worst excess {float((err - lim).max()):.3e}"
        assert is_poison16(hi[:, batch:]).all() and (lo[:, batch:] == -128).all(), f"{path}: write into slots >= batch"
    return path


@pytest.mark.parametrize("d,batch,expect", [(384, 1, "gemm_kernel<64,64>"), (512, 1, "gemm_kernel<128,128>"), (512, 3, "gemm256_kernel<mode 0>"),
                                            (1024, 1, "gemm256_kernel<mode 0>")])
def test_gemm_cross_kv_vs_fp64(kh, d, batch, expect):
    run_cross_kv(kh, d, 2, batch, batch + 1, expect=expect)


def test_gemm_cross_kv_split_vs_fp64(kh):
    run_cross_kv(kh, 768, 2, 3, 3, split=True, expect="gemm256_split_kernel<mode 0>")


def test_gemm_cross_kv_hr24_edges(kh):
    """A = 0: every output is its bias exactly, chosen at the hr24 edges - values just inside half an f16 ulp from hi (|r| -> 128, the
    clamp to 127), f16 subnormal hi, exact f16 values, zero"""
    d, L, batch = 384, 2, 1
    N = L * 2 * d
    rng = np.random.default_rng(17)
    hi = rng.uniform(0.5, 60.0, N).astype(np.float16).astype(np.float64) * rng.choice([-1.0, 1.0], N)
    ulp = np.spacing(np.abs(hi).astype(np.float16)).astype(np.float64)
    frac = rng.choice([0.5 - 2.0 ** -9, -0.5 + 2.0 ** -9, 0.4999, 0.25, 0.0, 127.6 / 256, -127.6 / 256], N)
    x = hi + frac * ulp
    sub = rng.random(N) < 0.25         # subnormal hi: |x| < 2^-14
    x[sub] = rng.uniform(-2.0 ** -14, 2.0 ** -14, int(sub.sum()))
    x[:4] = [0.0, 2.0 ** -24 * 0.75, -(2.0 ** -14) * 0.999, 65000.0]
    A = np.zeros((batch * CTX, d), np.float16)
    run_cross_kv(kh, d, L, batch, batch, A=A, bias=x.astype(np.float32), expect="gemm_kernel<64,64>")


# production shapes of every encoder GEMM at d in {384, 512, 1024, 1280}, batches 1 and 3
def _production(name):
    dims = weights.MODEL_DIMS[name]
    return [(name, b, s[0]) for b in (1, 3) for s in KH.encoder_shapes(dims, b)]


PRODUCTION = sum((_production(n) for n in ("test-tiny-en-l2", "test-base-l2", "test-medium-l2", "test-large-v3-l2")), [])


@pytest.mark.parametrize("name,batch,which", PRODUCTION, ids=[f"{n}-b{b}-{w}" for n, b, w in PRODUCTION])
def test_gemm_production_shapes_vs_fp64(kh, name, batch, which):
    dims = weights.MODEL_DIMS[name]
    d = dims.n_audio_state
    if which == "conv1":
        run_conv1(kh, dims.n_mels, d, batch)
    elif which == "conv2":
        run_conv2(kh, d, batch)
    elif which == "qkv":
        run_qkv(kh, d, batch)
    elif which == "cross_kv":
        run_cross_kv(kh, d, dims.n_text_layer, batch, batch + 1)
    else:
        _, epi, M, N, K, _, _ = next(s for s in KH.encoder_shapes(dims, batch) if s[0] == which)
        run_rowmajor(kh, Gemm(epi, M, N, K, seed=M + N + K))


def _f16_launch(kh, g, off=0):
    out = poison16((g.M, g.N))
    lo = poison16((g.M, g.N)) if g.split and g.epi == EPI_GELU_F16 else None
    ok(g.launch(kh, dict(out16=out, out16_lo=lo), g.N, offsets=dict(out16=off, out16_lo=off)))
    return out, lo


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("epi", [EPI_F16, EPI_GELU_F16, EPI_F32])
def test_gemm256_rows_equal_gemm64_rows_bit_for_bit(kh, epi, split):
    """gemm.hip: the 256 tile accumulates the k-steps of a tile in the order of gemm_kernel, so a chunk encodes to the same bits alone
    (64 x 64 tiles) or in a large batch (256 x 256, staged or direct epilogue); the split kernels keep the same promise"""
    M_big, M_small, N, K = 4500, 1500, 1536, 1280
    big = Gemm(epi, M_big, N, K, seed=21, split=split)
    small = Gemm(epi, M_small, N, K, seed=21, split=split)
    small.A, small.W, small.bias = np.ascontiguousarray(big.A[:M_small]), big.W, big.bias
    if split:
        small.A_lo = np.ascontiguousarray(big.A_lo[:M_small])
    pre = "gemm_split_kernel" if split else "gemm_kernel"
    assert small.path(N) == f"{pre}<64,64>"
    if epi == EPI_F32:
        assert big.path(N).endswith("<mode 0>")
        ob, os_ = poison32((M_big, N)), poison32((M_small, N))
        ok(big.launch(kh, dict(out32=ob), N))
        ok(small.launch(kh, dict(out32=os_), N))
        np.testing.assert_array_equal(ob[:M_small], os_)
        return
    assert big.path(N).endswith("<mode 1>") and big.path(N, out_align=8).endswith("<mode 0>")
    staged, staged_lo = _f16_launch(kh, big)
    direct, direct_lo = _f16_launch(kh, big, off=8)
    one, one_lo = _f16_launch(kh, small)
    np.testing.assert_array_equal(staged.view(np.uint16)[:M_small], one.view(np.uint16))
    np.testing.assert_array_equal(direct.view(np.uint16), staged.view(np.uint16))
    if staged_lo is not None:
        np.testing.assert_array_equal(staged_lo.view(np.uint16)[:M_small], one_lo.view(np.uint16))
        np.testing.assert_array_equal(direct_lo.view(np.uint16), staged_lo.view(np.uint16))


def test_f32_to_f16_split_vs_fp64(kh):
    rng = np.random.default_rng(23)
    x = np.concatenate([rng.standard_normal(100_000) * 50, np.exp(rng.uniform(-30, 5, 50_000)) * rng.choice([-1, 1], 50_000),
                        [0.0, 2.0 ** -24, -2.0 ** -14, 65504.0]]).astype(np.float32)
    hi, lo = poison16(x.shape), poison16(x.shape)
    ok(kh.f32_to_f16_split(x, hi, lo))
    np.testing.assert_array_equal(hi, x.astype(np.float16))
    check_split(hi, lo, x.astype(np.float64), 0.0, "f32_to_f16_split")


# ---------------------------------------------------------------------------------------------- LayerNorm
def ln_rows(rng, rows, d):
    """row kinds: plain, mean 10^3 x the spread (a one-pass variance loses it), constant, 30 - 50 x outlier channels"""
    x = 0.3 + rng.standard_normal((rows, d))
    kind = np.arange(rows) % 4
    x[kind == 1] = 1000.0 * rng.choice([-1.0, 1.0], ((kind == 1).sum(), 1)) + rng.standard_normal(((kind == 1).sum(), d))
    x[kind == 2] = rng.uniform(-3, 3, ((kind == 2).sum(), 1))
    out_ch = rng.choice(d, 6, replace=False)
    x[np.ix_(kind == 3, out_ch)] += rng.uniform(30, 50, 6) * rng.choice([-1.0, 1.0], 6)
    return x.astype(np.float32)


def ln_reference(x, g, b, d):
    """fp64 LayerNorm and its bound: the fp32 mean and the two-pass sum of squares are reduction trees of depth D <= d / 64 + 8 over the
    row (|delta mean| <= D u sum|x| / d, variance relative error <= (D + 3) u, rsqrt 2 u), then (x - mean) rstd g + b with 4 roundings"""
    x64 = x.astype(np.float64)
    mean = x64.mean(1, keepdims=True)
    var = ((x64 - mean) ** 2).mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + 1e-5)
    y = (x64 - mean) * rstd * g.astype(np.float64) + b.astype(np.float64)
    D = -(-d // 64) + 8
    dmean = D * U * np.abs(x64).sum(1, keepdims=True) / d
    bound = np.abs(g.astype(np.float64)) * rstd * (dmean + np.abs(x64 - mean) * ((D + 3) / 2 + 6) * U) + 4 * U * (np.abs(y) + np.abs(b))
    return y, bound


LN_WIDTHS = [64, 192, 384, 512, 768, 1024, 1280]


@pytest.mark.parametrize("lo", [False, True], ids=["f16", "f16-lo"])
@pytest.mark.parametrize("d", LN_WIDTHS)
def test_layernorm_v4_and_scalar_vs_fp64(kh, d, lo):
    rng = np.random.default_rng(d + lo)
    rows = 1002 + d % 3            # not a multiple of 4
    x = ln_rows(rng, rows, d)
    g = (1.0 + 0.3 * rng.standard_normal(d)).astype(np.float32)
    b = (0.2 + 0.5 * rng.standard_normal(d)).astype(np.float32)
    ref, bound = ln_reference(x, g, b, d)
    outs = {}
    for path, x_off in (("layernorm_v4_kernel<NT>", 0), ("layernorm_kernel", 8)):
        # the scalar kernel: an x view 8 bytes into its allocation (16-byte loads are off)
        assert KH.layernorm_path(d, x_align=16 if x_off == 0 else 8, has_lo=lo) == path
        y16, y32 = poison16((rows, d)), poison32((rows, d))
        y16_lo = poison16((rows, d)) if lo else None
        ok(kh.layernorm(rows, d, x, g, b, y16=y16, y32=y32, y16_lo=y16_lo, offsets=dict(x=x_off)))
        check_f32(y32, ref, bound, f"{path} y32 d={d}")
        check_f16(y16, ref, bound, f"{path} y16 d={d}")
        np.testing.assert_array_equal(y16, y32.astype(np.float16))
        if lo:
            check_split(y16, y16_lo, ref, bound, f"{path} y16 + lo d={d}")
            np.testing.assert_array_equal(y16_lo, (y32 - y16.astype(np.float32)).astype(np.float16))
        # without the f32 copy (the encoder's form)
        y16b = poison16((rows, d))
        y16b_lo = poison16((rows, d)) if lo else None
        ok(kh.layernorm(rows, d, x, g, b, y16=y16b, y16_lo=y16b_lo, offsets=dict(x=x_off)))
        np.testing.assert_array_equal(y16b.view(np.uint16), y16.view(np.uint16))
        if lo:
            np.testing.assert_array_equal(y16b_lo.view(np.uint16), y16_lo.view(np.uint16))
        outs[path] = y16
    # the two forms agree to 1 f16 ulp on the plain and the outlier rows - an ulp taken at max(|y|, 2^-10): their fp32
    # statistics differ in the last bits, which moves an output by ~1e-7, more than an f16 ulp only below 2^-10 (ulp 2^-20).  Not on
    # the mean-10^3 rows (kind 1) and the constant rows (kind 2): there the output is the last bits of the fp32 mean amplified by rstd
    # (up to 1 / sqrt(1e-5) = 316 on a constant row), which the two reduction orders round differently - both forms are held to the
    # fp64 bound above on those rows instead.
    a, c = outs["layernorm_v4_kernel<NT>"].astype(np.float64), outs["layernorm_kernel"].astype(np.float64)
    kind = np.arange(rows) % 4
    rows_ok = (kind == 0) | (kind == 3)
    ulp = 2.0 * KH.f16_half_ulp(np.maximum(np.maximum(np.abs(a), np.abs(c)), 2.0 ** -10))
    bad = (np.abs(a - c) > ulp)[rows_ok]
    assert not bad.any(), f"scalar vs v4: {int(bad.sum())} elements differ by more than 1 f16 ulp"


# ---------------------------------------------------------------------------------------------- encoder attention (v2)
PATTERNS = ("random", "rise_under_8", "rise_over_8", "dominant_first", "dominant_last", "uniform", "large")


def score_keys(rng, pattern):
    """channel-0 key values (the query's channel 0 is 1): the score pattern of one (batch, head)"""
    j = np.arange(CTX)
    if pattern == "rise_under_8":       # tile maxima rising by 7.875 per 64-key tile: the lazy rescale just holds off
        return 7.875 * (j // 64) - rng.uniform(0, 4, CTX) * (j % 64 != 17)
    if pattern == "rise_over_8":
        return 8.125 * (j // 64) - rng.uniform(0, 4, CTX) * (j % 64 != 17)
    if pattern == "dominant_first":
        s = rng.uniform(-1, 1, CTX); s[0] = 24.0; return s
    if pattern == "dominant_last":      # the last valid key, in the masked last tile
        s = rng.uniform(-1, 1, CTX); s[CTX - 1] = 24.0; return s
    if pattern == "uniform":
        return np.zeros(CTX)
    if pattern == "large":
        return rng.uniform(-120, 120, CTX)
    return rng.standard_normal(CTX)


def attention_case(batch, H, seed):
    d = 64 * H
    rng = np.random.default_rng(seed)
    q = np.zeros((batch, CTX, H, 64)); k = np.zeros((batch, CTX, H, 64))
    pats = []
    for b in range(batch):
        for h in range(H):
            p = PATTERNS[(b * H + h + seed) % len(PATTERNS)]
            pats.append(p)
            q[b, :, h, 0] = 1.0
            if p not in ("uniform", "rise_under_8", "rise_over_8"):     # (the rise patterns' tile maxima are exact)
                q[b, :, h, 1:] = 0.1 * rng.standard_normal((CTX, 63)) + 0.02 * (h + 1)
                k[b, :, h, 1:] = 0.3 * rng.standard_normal((CTX, 63))
            k[b, :, h, 0] = score_keys(rng, p)
    v = (0.1 * (np.arange(batch * H).reshape(batch, H, 1, 1) % 5) + rng.standard_normal((batch, H, 64, CTX))).astype(np.float16)
    vt = np.full((batch, H, 64, CTX_PAD), 1.0e4, np.float16)      # the pad keys 1500 .. 1535: large and finite (masked to weight 0)
    vt[..., :CTX] = v
    return (q.reshape(batch * CTX, d).astype(np.float16), k.reshape(batch * CTX, d).astype(np.float16),
            np.ascontiguousarray(vt.reshape(batch, d, CTX_PAD)), pats)


def attention_reference(q, k, vt, batch, H):
    """fp64 softmax(q k^T) v per (batch, head) and its bound.  The kernel's weights are p_j = exp(s_j - m) with m <= max s (the lazy
    rescale keeps m within 8 of every tile maximum: p_j <= e^8), rounded to f16 for P V (relative 2^-11 per weight, 2^-25 absolute
    below the f16 normal range) while l = sum p_j stays fp32.  With e_j the relative error of p_j from its score (MFMA fp32 sum of 64 exact
    f16 products: 2 * 64 u sum_c |q_c k_jc|; the exp2 argument fma(s, log2 e, -m log2 e): 4 u (|s_j| + |m|) + 4 u) and n u for the
    fp32 sums over n = 1500 keys,
        |out - ref| <= (sum_j p_j |v_j| (2^-11 + 2 e_j + n u) + 2^-25 sum_j |v_j|) / l + |ref| (2 max_j e_j + n u) + half an f16 ulp.
    """
    d = 64 * H
    Q = q.astype(np.float64).reshape(batch, CTX, H, 64)
    Kx = k.astype(np.float64).reshape(batch, CTX, H, 64)
    V = vt.astype(np.float64).reshape(batch, H, 64, CTX_PAD)[..., :CTX]
    ref = np.zeros((batch, CTX, H, 64)); bound = np.zeros_like(ref)
    n = CTX
    for b in range(batch):
        for h in range(H):
            qa, ka, va = Q[b, :, h], Kx[b, :, h], V[b, h].T           # [1500][64], [1500][64], [1500 keys][64]
            s = qa @ ka.T
            m = s.max(1, keepdims=True)
            p = np.exp(s - m)
            l = p.sum(1, keepdims=True)
            o = p @ va / l
            e = 128 * U * (np.abs(qa) @ np.abs(ka).T) + 4 * U * (np.abs(s) + np.abs(m)) + 4 * U
            av = np.abs(va)
            bd = ((p * (2.0 ** -11 + 2 * e + n * U)) @ av + 2.0 ** -25 * av.sum(0, keepdims=True)) / l
            bd += np.abs(o) * (2 * e.max(1, keepdims=True) + n * U)
            ref[b, :, h], bound[b, :, h] = o, bd
    return ref.reshape(batch * CTX, d), bound.reshape(batch * CTX, d)


@pytest.mark.parametrize("lo", [False, True], ids=["f16", "f16-lo"])
@pytest.mark.parametrize("batch,H", [(1, 1), (3, 6), (1, 8), (1, 16), (3, 20)])
def test_encoder_attention_v2_vs_fp64(kh, batch, H, lo):
    d = 64 * H
    q, k, vt, pats = attention_case(batch, H, seed=31 * H + batch + lo)
    out = poison16((batch * CTX, d))
    out_lo = poison16((batch * CTX, d)) if lo else None
    ok(kh.encoder_attention(batch, H, d, q, k, vt, out, out_lo))
    ref, bound = attention_reference(q, k, vt, batch, H)
    if lo:
        check_split(out, out_lo, ref, bound, f"encoder_attention_v2 B={batch} H={H}")
    else:
        assert not is_poison16(out).any(), "attention outputs never written"
        err = np.abs(out.astype(np.float64) - ref)
        lim = bound + KH.f16_half_ulp(np.abs(ref) + bound)
        bad = (err > lim).reshape(batch, CTX, H, 64).any(axis=(1, 3))
        assert not bad.any(), ("out of bound in (batch, head, pattern)", [(b, h, pats[b * H + h]) for b, h in zip(*np.nonzero(bad))],
                               float((err - lim).max()))
    for i, p in enumerate(pats):       # the patterns' closed forms: uniform scores average V; a dominant key returns its own row
        b, h = divmod(i, H)
        rows = slice(b * CTX, (b + 1) * CTX)
        got = out[rows, h * 64:(h + 1) * 64].astype(np.float64)
        if p == "uniform":
            np.testing.assert_allclose(got, np.broadcast_to(vt[b, h * 64:(h + 1) * 64, :CTX].astype(np.float64).mean(1), got.shape), atol=2e-3)
        if p in ("dominant_first", "dominant_last"):
            key = 0 if p == "dominant_first" else CTX - 1
            np.testing.assert_allclose(got, np.broadcast_to(vt[b, h * 64:(h + 1) * 64, key].astype(np.float64), got.shape), atol=2e-3, rtol=2e-3)
