"""ctypes side of tests/native/kernel_harness.hip (one launcher of csrc/kernels.h per call, host buffers in and out, guard bands and
poison) and a Python restatement of the launchers' kernel choice (csrc/launch_plan.h gemm_plan / layernorm_plan, the functions
csrc/gemm.hip launch_epi and csrc/layernorm.hip launch_layernorm switch on) that labels every case with the kernel it is meant to reach;
plan_check_build / plan_check_run put the real planners behind it (tests/native/launch_plan_check.cpp, g++).  Used by
tests/test_gpu_kernels.py (device) and tests/test_kernel_harness.py, tests/test_launch_plan.py (CPU: build, exports, predicates)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "kernel_harness.hip")
LIBDIR = os.path.join(ROOT, "whisperkit_amd")
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")

EXPORTS = ("kh_gemm", "kh_gemm_buffer_count", "kh_guard_bytes", "kh_layernorm", "kh_encoder_attention", "kh_f32_to_f16_split")

# csrc/kernels.h GemmEpi
EPI_F16, EPI_GELU_F16, EPI_RESID_F32, EPI_QKV_ENC, EPI_CONV1, EPI_CONV2, EPI_F32, EPI_CROSS_KV = range(8)
STAGED_EPIS = (EPI_F16, EPI_GELU_F16, EPI_RESID_F32, EPI_QKV_ENC)      # gemm.hip kHasStagedEpilogue
# csrc/common.h
CTX, CTX_PAD, FRAMES, FRAMES_PAD = 1500, 1536, 3000, 3002

GUARD_POISON_F16 = np.uint16(0x7E00)     # f16 NaN


class KhBuf(C.Structure):
    _fields_ = [("host", C.c_void_p), ("bytes", C.c_longlong), ("offset", C.c_longlong), ("is_out", C.c_int), ("pad_", C.c_int)]


class KhGemmArgs(C.Structure):
    _fields_ = [("epi", C.c_int), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("lda", C.c_int), ("a_rows_per_batch", C.c_int),
                ("a_batch_stride", C.c_longlong), ("ldc", C.c_int), ("d_model", C.c_int), ("rows_per_batch_out", C.c_int),
                ("max_batch", C.c_int)]


GEMM_SLOTS = ("A", "A_lo", "W", "bias", "pos", "out16", "out32", "k16", "vt16", "out16_lo", "kv_k_hi", "kv_v_hi", "kv_k_lo", "kv_v_lo")
GEMM_OUTS = ("out16", "out32", "k16", "vt16", "out16_lo", "kv_k_hi", "kv_v_hi", "kv_k_lo", "kv_v_lo")


def build(outdir):
    """hipcc the harness into outdir against the in-tree libwhisperhip.so; returns the library path"""
    lib = os.path.join(str(outdir), "libkernel_harness.so")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", "-Wno-unused-result",
                    "-I", os.path.join(ROOT, "whisperkit_amd", "csrc"), "-I", os.path.join(ROOT, "include"), SRC,
                    "-L", LIBDIR, "-lwhisperhip", "-Wl,-rpath," + LIBDIR, "-o", lib], check=True)
    return lib


def plan_check_build(outdir):
    """g++ tests/native/launch_plan_check.cpp against csrc/launch_plan.h and csrc/knobs.h; returns the program's path"""
    exe = os.path.join(str(outdir), "launch_plan_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "whisperkit_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "launch_plan_check.cpp"), "-o", exe], check=True)
    return exe


def plan_check_run(exe, lines):
    """one request line in, one answer line out (the protocol: the head of launch_plan_check.cpp)"""
    lines = list(lines)
    out = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
    got = out.stdout.splitlines()
    assert out.returncode == 0 and len(got) == len(lines) and not any(g.startswith("ERROR") for g in got), (out.stdout[-2000:], out.stderr[-2000:])
    return got


def gemm_request(M, N, K, lda=None, a_batch_stride=0, ldc=None, d_model=0, epi=EPI_F16, split=False, out_align=16, epi_mode=1):
    """the launch_plan_check line of gemm_path's arguments: an output base that out_align divides and 2 out_align does not; no persistent loop"""
    return f"gemm {M} {N} {K} {K if lda is None else lda} {a_batch_stride} {N if ldc is None else ldc} {d_model} {epi} {int(split)} {out_align} {epi_mode} 0 0 0 256"


def layernorm_request(d, x_align=16, gb_align=16, y32_align=16, y16_align=8, lo_align=8, has_lo=False, v4=2):
    return f"ln {d} {x_align | gb_align | y32_align} {y16_align} {lo_align if has_lo else 0} {int(has_lo)} {v4}"


class Harness:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        for name in ("kh_gemm", "kh_layernorm", "kh_encoder_attention", "kh_f32_to_f16_split"):
            getattr(self.lib, name).restype = C.c_int
        self.lib.kh_gemm.argtypes = [C.POINTER(KhGemmArgs), C.POINTER(KhBuf), C.POINTER(C.c_longlong)]
        self.lib.kh_layernorm.argtypes = [C.c_int, C.c_int, C.POINTER(KhBuf), C.POINTER(C.c_longlong)]
        self.lib.kh_encoder_attention.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(KhBuf), C.POINTER(C.c_longlong)]
        self.lib.kh_f32_to_f16_split.argtypes = [C.c_longlong, C.POINTER(KhBuf), C.POINTER(C.c_longlong)]
        self.lib.kh_guard_bytes.restype = C.c_longlong
        assert self.lib.kh_gemm_buffer_count() == len(GEMM_SLOTS)

    @staticmethod
    def _bufs(arrays, names, outs, offsets):
        """KhBuf array over contiguous numpy arrays (None -> null); the arrays stay owned by the caller"""
        bufs = (KhBuf * len(names))()
        for i, n in enumerate(names):
            a = arrays.get(n)
            if a is None:
                continue
            assert a.flags.c_contiguous
            bufs[i] = KhBuf(a.ctypes.data, a.nbytes, int(offsets.get(n, 0)), int(n in outs), 0)
        return bufs

    def _call(self, fn, *args):
        guard = C.c_longlong(-1)
        status = fn(*args, C.byref(guard))
        return int(status), int(guard.value)

    def gemm(self, epi, M, N, K, lda, ldc, arrays, a_rows_per_batch=None, a_batch_stride=0, d_model=0, rows_per_batch_out=0,
             max_batch=0, offsets=None):
        """wh::launch_gemm over host arrays (outputs updated in place); returns (hip status, changed guard bytes)"""
        s = KhGemmArgs(epi, M, N, K, lda, M if a_rows_per_batch is None else a_rows_per_batch, a_batch_stride, ldc, d_model,
                       rows_per_batch_out, max_batch)
        bufs = self._bufs(arrays, GEMM_SLOTS, GEMM_OUTS, offsets or {})
        return self._call(self.lib.kh_gemm, C.byref(s), bufs)

    def layernorm(self, rows, d, x, g, b, y16=None, y32=None, y16_lo=None, offsets=None):
        names = ("x", "g", "b", "y16", "y32", "y16_lo")
        bufs = self._bufs(dict(x=x, g=g, b=b, y16=y16, y32=y32, y16_lo=y16_lo), names, ("y16", "y32", "y16_lo"), offsets or {})
        return self._call(self.lib.kh_layernorm, rows, d, bufs)

    def encoder_attention(self, batch, n_head, d, q, k, vt, out, out_lo=None):
        names = ("q", "k", "vt", "out", "out_lo")
        bufs = self._bufs(dict(q=q, k=k, vt=vt, out=out, out_lo=out_lo), names, ("out", "out_lo"), {})
        return self._call(self.lib.kh_encoder_attention, batch, n_head, d, bufs)

    def f32_to_f16_split(self, x, hi, lo):
        bufs = self._bufs(dict(x=x, hi=hi, lo=lo), ("x", "hi", "lo"), ("hi", "lo"), {})
        return self._call(self.lib.kh_f32_to_f16_split, x.size, bufs)


# ---------------------------------------------------------------------------------------------- the launchers' kernel choice, restated
def gemm_path(M, N, K, lda=None, a_batch_stride=0, ldc=None, d_model=0, epi=EPI_F16, split=False, out_align=16, epi_mode=1):
    """The kernel launch_epi picks for the Float16 (split=False) / split (split=True) A operand with the default environment
    (epi_mode = WH_GEMM_EPI_MODE = 1, no persistent loop).  out_align: the largest power of two (<= 16) that divides every output base address."""
    lda = K if lda is None else lda
    ldc = N if ldc is None else ldc
    tiles256 = -(-M // 256) * -(-N // 256)
    kt = 32 if split else 64
    if tiles256 >= 64 and K % kt == 0 and lda % 8 == 0 and a_batch_stride % 8 == 0 and N % 4 == 0:
        name = "gemm256_split_kernel" if split else "gemm256_kernel"
        staged = (epi in STAGED_EPIS and out_align % 16 == 0 and N % 64 == 0 and M % 4 == 0 and ldc % 8 == 0 and d_model % 64 == 0)
        return f"{name}<mode {epi_mode if staged and epi_mode in (1, 2) else 0}>"
    tiles128 = -(-M // 128) * -(-N // 128)
    name = "gemm_split_kernel" if split else "gemm_kernel"
    return f"{name}<128,128>" if tiles128 >= 192 else f"{name}<64,64>"


def layernorm_path(d, x_align=16, gb_align=16, y32_align=16, y16_align=8, lo_align=8, has_lo=False, v4=2):
    """The kernel launch_layernorm picks with the default environment (v4 = WH_LN_V4 = 2: the non-temporal vector form; 1: the plain
    vector form; 0: the scalar kernel)"""
    aligned = d % 4 == 0 and min(x_align, gb_align, y32_align) % 16 == 0 and y16_align % 8 == 0
    if has_lo:
        aligned = aligned and lo_align % 8 == 0
    if not aligned or v4 == 0:
        return "layernorm_kernel"
    return "layernorm_v4_kernel<NT>" if v4 == 2 else "layernorm_v4_kernel"


def encoder_shapes(dims, batch):
    """(label, epi, M, N, K, lda, a_batch_stride) of every encoder GEMM of one wh_encode_features call (csrc/capi.hip)"""
    d, nm, L = dims.n_audio_state, dims.n_mels, dims.n_text_layer
    M = batch * CTX
    return [("conv1", EPI_CONV1, batch * FRAMES, d, 3 * nm, nm, FRAMES_PAD * nm),
            ("conv2", EPI_CONV2, M, d, 3 * d, 2 * d, FRAMES_PAD * d),
            ("qkv", EPI_QKV_ENC, M, 3 * d, d, d, 0),
            ("out", EPI_RESID_F32, M, d, d, d, 0),
            ("fc1", EPI_GELU_F16, M, 4 * d, d, d, 0),
            ("fc2", EPI_RESID_F32, M, d, 4 * d, 4 * d, 0),
            ("cross_kv", EPI_CROSS_KV, M, L * 2 * d, d, d, 0)]


# ---------------------------------------------------------------------------------------------- numerics shared by the tests
def f16_half_ulp(x):
    """half a Float16 ulp at |x| (2^-25 below the normal range)"""
    e = np.floor(np.log2(np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -14)))
    return 2.0 ** (e - 11)


# max |gelu_f32(x) - gelu_f64(x)| / max(1, |x|) over x in [-64, 64] (test_kernel_harness.py re-measures it); the device tests allow twice this
GELU_FAST_ERR_MEASURED = 1.8e-7


def gelu_f32(x):
    """float32 restatement of csrc/common.h gelu_erf_fast (the hardware reciprocal and exp are taken as correctly rounded)"""
    x = np.asarray(x, np.float32)
    f = np.float32
    ax = np.abs(x) * f(0.70710678118654752440)
    t = f(1.0) / (f(0.3275911) * ax + f(1.0))
    p = f(1.061405429) * t + f(-1.453152027)
    p = p * t + f(1.421413741)
    p = p * t + f(-0.284496736)
    p = p * t + f(0.254829592)
    q = p * t * np.exp(-ax * ax)
    return f(0.5) * x * np.where(x >= 0, f(2.0) - q, q)


def gelu_f64(x):
    from scipy.special import erf
    x = np.asarray(x, np.float64)
    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


def hr24_unit(hi_bits):
    """csrc/kernels.h hr24_unit: ulp(hi) / 256 = 2^(e - 33), e the biased exponent of hi (subnormals: e = 1)"""
    e = (np.asarray(hi_bits, np.uint32) >> 10) & 31
    return np.exp2(np.maximum(e, 1).astype(np.float64) - 33.0)
