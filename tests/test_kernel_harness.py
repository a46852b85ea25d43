"""CPU checks of the kernel-level test harness (tests/native/kernel_harness.hip, tests/kernel_harness.py): it builds against the in-tree
library, exports its entry points, fails with a HIP status instead of crashing where there is no GPU, and its restatement of the
launchers' kernel choice agrees with csrc/gemm.hip / csrc/layernorm.hip on the production shapes of every preset.  The device side:
tests/test_gpu_kernels.py."""
import os
import re

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


def test_dispatch_restatement_matches_the_launcher_source():
    """the predicates kernel_harness.gemm_path / layernorm_path restate, as they stand in the launchers"""
    src = re.sub(r"\s+", " ", open(os.path.join(KH.ROOT, "whisperkit_amd", "csrc", "gemm.hip")).read())
    assert "tiles256 >= 64 && a.K % 64 == 0 && a.lda % 8 == 0 && a.a_batch_stride % 8 == 0 && a.N % 4 == 0" in src
    assert "tiles256 >= 64 && a.K % 32 == 0 && a.lda % 8 == 0 && a.a_batch_stride % 8 == 0 && a.N % 4 == 0" in src
    assert src.count("shape_ok = aligned && a.N % 64 == 0 && a.M % 4 == 0 && a.ldc % 8 == 0 && a.d_model % 64 == 0") == 2
    assert src.count("if (tiles128 >= 192)") == 2
    assert "EPI == EPI_F16 || EPI == EPI_GELU_F16 || EPI == EPI_RESID_F32 || EPI == EPI_QKV_ENC" in src
    ln = re.sub(r"\s+", " ", open(os.path.join(KH.ROOT, "whisperkit_amd", "csrc", "layernorm.hip")).read())
    assert ("aligned = d % 4 == 0 && (((uintptr_t)x | (uintptr_t)g | (uintptr_t)b | (uintptr_t)y32) % 16) == 0 && "
            "((uintptr_t)y16 % 8) == 0") in ln


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
