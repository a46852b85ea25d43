"""CPU checks of the kernel-level test harness (tests/native/kernel_harness.hip, tests/kernel_harness.py): it builds against the in-tree
library, exports its entry points, fails with a HIP status instead of crashing where there is no GPU, and its restatement of the
launchers' kernel choice agrees with csrc/launch_plan.h (the planners csrc/gemm.hip / csrc/layernorm.hip switch on) on the production
shapes of every preset and on every case of the device tests.  The device side:
tests/test_gpu_kernels.py."""
import os

import numpy as np
import pytest

import kernel_harness as KH
from kernel_harness import EPI_CONV1, EPI_CONV2, EPI_CROSS_KV, EPI_F16, EPI_GELU_F16, EPI_QKV_ENC, EPI_RESID_F32
from whisperkit_amd import weights


@pytest.fixture(scope="module")
def kh(tmp_path_factory):
    return KH.Harness(KH.build(tmp_path_factory.mktemp("kernel_harness_cpu")))


def test_harness_builds_and_exports_its_entry_points(kh):
    for name in KH.EXPORTS:
        assert hasattr(kh.lib, name), name
    assert kh.lib.kh_gemm_buffer_count() == len(KH.GEMM_SLOTS) == 14
    assert kh.lib.kh_guard_bytes() >= 4096


def test_harness_returns_a_hip_status_instead_of_crashing(kh):
    x = np.ones((4, 64), np.float32)
    g, b = np.ones(64, np.float32), np.zeros(64, np.float32)
    y = np.zeros((4, 64), np.float16)
    # offsets that are not multiples of 8 are refused before anything touches a device (hipErrorInvalidValue = 1)
    assert kh.layernorm(4, 64, x, g, b, y16=y, offsets=dict(x=4)) == (1, 0)
    if not os.path.exists("/dev/kfd"):      # no GPU on this host: the allocation fails and the wrapper reports it
        status, _ = kh.layernorm(4, 64, x, g, b, y16=y)
        assert status != 0
        status, _ = kh.gemm(EPI_F16, 64, 64, 64, 64, 64, dict(A=np.ones((64, 64), np.float16), W=np.ones((64, 64), np.float16),
                                                              out16=np.zeros((64, 64), np.float16)))
        assert status != 0


def _gpu_kernel_cases():
    """(gemm_path keyword arguments, expected kernel or None) of every GEMM case tests/test_gpu_kernels.py constructs - read from its own
    case lists and parametrize marks; the shapes are those its run_* helpers build - and the arguments of its LayerNorm cases"""
    import test_gpu_kernels as G
    CTX, FRAMES, FRAMES_PAD = KH.CTX, KH.FRAMES, KH.FRAMES_PAD

    def params(fn):
        return [m.args[1] for m in fn.pytestmark if m.name == "parametrize"]

    def qkv(d, batch, off=0, split=False):
        return dict(M=batch * CTX, N=3 * d, K=d, ldc=d, d_model=d, epi=EPI_QKV_ENC, split=split, out_align=16 if off % 16 == 0 else 8)

    def conv1(n_mels, d, batch, split=False):
        return dict(M=batch * FRAMES, N=d, K=3 * n_mels, lda=n_mels, a_batch_stride=FRAMES_PAD * n_mels, ldc=d, epi=EPI_CONV1, split=split)

    def conv2(d, batch, split=False):
        return dict(M=batch * CTX, N=d, K=3 * d, lda=2 * d, a_batch_stride=FRAMES_PAD * d, ldc=d, epi=EPI_CONV2, split=split)

    def cross_kv(d, L, batch, split=False):
        return dict(M=batch * CTX, N=L * 2 * d, K=d, ldc=L * 2 * d, d_model=d, epi=EPI_CROSS_KV, split=split)

    gemms = []
    for epi, M, N, K, ldc, off, split, expect in G.ROWMAJOR_CASES:      # thresholds one step either side, unaligned bases, ldc padding
        gemms.append((dict(M=M, N=N, K=K, ldc=ldc, epi=epi, split=split, out_align=16 if off % 16 == 0 else 8), expect))
    gemms += [(qkv(d, b, off), e) for d, b, off, e in params(G.test_gemm_qkv_enc_layout_vs_fp64)[0]]
    gemms.append((qkv(768, 3, split=True), "gemm256_split_kernel<mode 1>"))
    gemms += [(conv1(nm, d, b), e) for nm, d, b, e in params(G.test_gemm_conv1_view_vs_fp64)[0]]
    gemms.append((conv1(128, 1280, 3, split=True), "gemm256_split_kernel<mode 0>"))
    gemms += [(conv2(d, b), e) for d, b, e in params(G.test_gemm_conv2_view_vs_fp64)[0]]
    gemms.append((conv2(1024, 3, split=True), "gemm256_split_kernel<mode 0>"))
    gemms += [(cross_kv(d, 2, b), e) for d, b, e in params(G.test_gemm_cross_kv_vs_fp64)[0]]
    gemms.append((cross_kv(768, 2, 3, split=True), "gemm256_split_kernel<mode 0>"))
    gemms.append((cross_kv(384, 2, 1), "gemm_kernel<64,64>"))           # test_gemm_cross_kv_hr24_edges
    for name, batch, which in G.PRODUCTION:
        dims = weights.MODEL_DIMS[name]
        _, epi, M, N, K, lda, stride = next(s for s in KH.encoder_shapes(dims, batch) if s[0] == which)
        gemms.append((dict(M=M, N=N, K=K, lda=lda, a_batch_stride=stride, ldc=N, d_model=dims.n_audio_state if epi in (EPI_QKV_ENC, EPI_CROSS_KV) else 0, epi=epi), None))
    for split in (False, True):                                          # test_gemm256_rows_equal_gemm64_rows_bit_for_bit
        for epi in (EPI_F16, EPI_GELU_F16, KH.EPI_F32):
            for M, align in ((4500, 16), (4500, 8), (1500, 16)):
                gemms.append((dict(M=M, N=1536, K=1280, epi=epi, split=split, out_align=align), None))
    lns = [dict(d=d, x_align=xa, has_lo=lo) for d in G.LN_WIDTHS for lo in (False, True) for xa in (16, 8)]
    return gemms, lns


def test_dispatch_restatement_matches_the_launch_planners(tmp_path):
    """kernel_harness.gemm_path / layernorm_path against the functions the launchers switch on (csrc/launch_plan.h through
    tests/native/launch_plan_check.cpp): every preset x batch x operand form, every case of tests/test_gpu_kernels.py, every epilogue mode
    and every LayerNorm form"""
    exe = KH.plan_check_build(tmp_path)
    gemms, lns = _gpu_kernel_cases()
    assert len(gemms) > 100 and len(lns) == 28
    for name, dims in sorted(weights.MODEL_DIMS.items()):
        for batch in (1, 3, 32):
            for which, epi, M, N, K, lda, stride in KH.encoder_shapes(dims, batch):
                for split in (False, True):
                    gemms.append((dict(M=M, N=N, K=K, lda=lda, a_batch_stride=stride, ldc=N,
                                       d_model=dims.n_audio_state if epi in (EPI_QKV_ENC, EPI_CROSS_KV) else 0, epi=epi, split=split), None))
        d = dims.n_audio_state
        lns += [dict(d=d), dict(d=d, has_lo=True), dict(d=d, x_align=8), dict(d=d, y16_align=4), dict(d=d, lo_align=4, has_lo=True), dict(d=d, gb_align=8),
                dict(d=d, y32_align=4), dict(d=d, lo_align=4)]
    lns += [dict(d=130), dict(d=66, has_lo=True)]                        # d % 4 != 0
    asked, want = [], []
    for kw, expect in gemms:
        for epi_mode in (0, 1, 2):
            asked.append(KH.gemm_request(epi_mode=epi_mode, **kw))
            want.append(KH.gemm_path(epi_mode=epi_mode, **kw))
            if expect is not None and epi_mode == 1:
                assert want[-1].startswith(expect), (kw, want[-1], expect)
    for kw in lns:
        for v4 in (0, 1, 2):
            asked.append(KH.layernorm_request(v4=v4, **kw))
            want.append(KH.layernorm_path(v4=v4, **kw))
    got = KH.plan_check_run(exe, asked)
    for line, g, w in zip(asked, got, want):
        assert (g.split(" grid ")[0] if line.startswith("gemm") else g) == w, (line, g, w)
    assert {w for w in want if w.startswith("layernorm")} == {"layernorm_kernel", "layernorm_v4_kernel", "layernorm_v4_kernel<NT>"}
    for fam in ("gemm256_kernel<mode 0>", "gemm256_kernel<mode 1>", "gemm256_kernel<mode 2>", "gemm256_split_kernel<mode 2>", "gemm_kernel<128,128>",
                "gemm_split_kernel<64,64>"):
        assert fam in want, fam
    # the knobs the restatement leaves at their defaults: no 256 tile at all; the persistent loop for the Float16 operand form only, on
    # min(WH_GEMM_PERSIST_WGS or the CUs, the tiles rounded up to 8) workgroups
    big = "4500 1536 1280 1280 0 1536 0 0"
    got = KH.plan_check_run(exe, [f"gemm {big} 0 16 1 1 0 0 256", f"gemm {big} 0 16 1 0 1 0 256", f"gemm {big} 1 16 1 0 1 0 256",
                                  f"gemm {big} 0 16 1 0 1 64 256", f"gemm {big} 0 16 1 0 0 0 256", f"gemm {big} 0 8 2 0 1 0 256"])
    assert got == ["gemm_kernel<128,128> grid 12 36", "gemm256p_kernel<mode 1> grid 112 1", "gemm256_split_kernel<mode 1> grid 108 1",
                   "gemm256p_kernel<mode 1> grid 64 1", "gemm256_kernel<mode 1> grid 108 1", "gemm256p_kernel<mode 0> grid 112 1"]


# hand-derived kernel choices (tiles256 = ceil(M / 256) ceil(N / 256), tiles128 likewise)
EXPECTED = {
    ("test-tiny-en-l2", 1): dict(conv1="gemm_kernel<64,64>", conv2="gemm_kernel<64,64>", qkv="gemm_kernel<64,64>",
                                 out="gemm_kernel<64,64>", fc1="gemm_kernel<64,64>", fc2="gemm_kernel<64,64>", cross_kv="gemm_kernel<64,64>"),
    ("test-tiny-en-l2", 3): dict(conv1="gemm_kernel<128,128>", qkv="gemm256_kernel<mode 1>", fc1="gemm256_kernel<mode 1>",
                                 fc2="gemm_kernel<64,64>", cross_kv="gemm256_kernel<mode 0>"),
    ("test-large-v3-l2", 1): dict(conv1="gemm_kernel<128,128>", conv2="gemm_kernel<64,64>", qkv="gemm256_kernel<mode 1>",
                                  out="gemm_kernel<64,64>", fc1="gemm256_kernel<mode 1>", fc2="gemm_kernel<64,64>",
                                  cross_kv="gemm256_kernel<mode 0>"),
    ("test-large-v3-l2", 3): dict(conv1="gemm256_kernel<mode 0>", conv2="gemm256_kernel<mode 0>", out="gemm256_kernel<mode 1>",
                                  fc2="gemm256_kernel<mode 1>"),
    ("test-small-l2", 1): dict(conv1="gemm_kernel<64,64>", fc1="gemm256_kernel<mode 1>"),
}


@pytest.mark.parametrize("name", sorted(weights.MODEL_DIMS))
def test_dispatch_restatement_on_every_preset(name):
    dims = weights.MODEL_DIMS[name]
    for batch in (1, 3, 32):
        for which, epi, M, N, K, lda, stride in KH.encoder_shapes(dims, batch):
            path = KH.gemm_path(M, N, K, lda, stride, N, dims.n_audio_state if epi in (EPI_QKV_ENC, EPI_CROSS_KV) else 0, epi)
            split = KH.gemm_path(M, N, K, lda, stride, N, dims.n_audio_state if epi in (EPI_QKV_ENC, EPI_CROSS_KV) else 0, epi, split=True)
            exp = EXPECTED.get((name, batch), {}).get(which)
            if exp is not None:
                assert path == exp, (name, batch, which, path)
            t256 = -(-M // 256) * -(-N // 256)
            if path.startswith("gemm256"):
                assert t256 >= 64 and K % 64 == 0
                assert path.endswith("<mode 1>") == (epi in (EPI_F16, EPI_GELU_F16, EPI_RESID_F32, EPI_QKV_ENC))   # production shapes are aligned
                assert split.replace("_split", "") == path            # K % 64 == 0 implies K % 32 == 0
            else:
                assert t256 < 64 or K % 64 != 0
                if t256 >= 64:
                    assert epi == EPI_CONV1 and dims.n_mels == 80   # K = 240: the only production K that is not whole 64-wide tiles
                    assert split.startswith("gemm_split_kernel")     # ... nor whole 32-wide tiles
            if epi in (EPI_CONV1, EPI_CONV2, EPI_CROSS_KV):
                assert not path.endswith("<mode 1>")
    # LayerNorm: every production width takes the vector kernel; an unaligned view takes the scalar one
    d = dims.n_audio_state
    assert KH.layernorm_path(d) == KH.layernorm_path(d, has_lo=True) == "layernorm_v4_kernel<NT>"
    assert KH.layernorm_path(d, x_align=8) == KH.layernorm_path(d, y16_align=4) == "layernorm_kernel"
    assert KH.layernorm_path(d, lo_align=4, has_lo=True) == "layernorm_kernel"


def test_gelu_restatement_error_bound():
    """the float32 restatement of gelu_erf_fast against erf in fp64: the measured error the device GELU bounds take twice of"""
    x = np.concatenate([np.linspace(-64, 64, 2_000_001), np.random.default_rng(0).standard_normal(500_000) * 4]).astype(np.float32)
    e = np.abs(KH.gelu_f32(x).astype(np.float64) - KH.gelu_f64(x.astype(np.float64))) / np.maximum(1.0, np.abs(x))
    assert 1.0e-7 < e.max() <= KH.GELU_FAST_ERR_MEASURED


def test_hr24_unit_restatement():
    hi = np.array([1.0, 2.0, 0.5, 60000.0, 2.0 ** -14, 2.0 ** -20, 0.0], np.float16)
    np.testing.assert_array_equal(KH.hr24_unit(hi.view(np.uint16)),
                                  np.spacing(np.maximum(np.abs(hi), np.float16(2.0 ** -14))).astype(np.float64) / 256)
    np.testing.assert_array_equal(KH.f16_half_ulp([1.0, 1.5, 2.0 ** -20, 0.0]), [2.0 ** -11, 2.0 ** -11, 2.0 ** -25, 2.0 ** -25])
