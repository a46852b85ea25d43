"""Shared by tests/test_token_alternatives.py (CPU) and tests/test_gpu_token_alternatives.py (GPU): the numpy restatement of the token alternatives
(wh_session_set_token_alternatives), the rows the kernel-alone test feeds it, and the error bound derived from the fp32 operations of the
recording instantiation of sampler_kernel.  Nothing here looks at the library's output.

The restatement (float64): x_i = row_i / T at T != 0 (T as the float32 the device holds), row_i otherwise, over the FINITE entries; lp_i = x_i - lse;
the n best in descending order, ties to the lower id, padded with (-1, -inf); H = lse - sum(e^(x - m) x) / sum(e^(x - m)).

The bound (u = 2^-24).  The kernel: alpha = fl(1 / T), xs_i = fl(x_i alpha) (T != 0 only); m = max xs (exact); e_i = expf(fl(xs_i - m)); se = sum e_i and
sx = sum fl(e_i xs_i), each as 1024 strided accumulators in ascending i, six shuffle levels inside a wave, sixteen waves added one after the other;
lse = fl(m + logf(se)); lp_k = fl(xs_k - lse); H = fl(lse - fl(sx / se)).  With d_i = m - x_i >= 0, S = sum exp(-d_i), X = max |x_i|:
  * scaling: alpha and the product round once each, |xs_i - x_i| <= 2 u |x_i| <= a := 2 u X  (a = 0 at T = 0);
  * the exponent fl(xs_i - m) is off by <= 2 a + u d_i, expf by 2 ulp = 4 u relative (the HIP tables list 1 ulp; 2 are allowed, as in
    tests/test_gpu_no_speech.py), the sum by c := (ceil(V / 1024) - 1 + 6 + 16) u relative (positive terms):
    theta := c + 4 u + 2 a + u sum(d_i exp(-d_i)) / S is the relative error of se;
  * logf: 2 ulp = 4 u |log S|; the add rounds by u |lse|; m carries a:  err_lse := a + theta + 4 u |log S| + u |lse|;
  * lp_k: err_lse + a + u |lp_k|;
  * sx: every term is off by (4 u + 2 a + u d_i) from e_i, 2 u from xs_i, u from the product (or less, fused) and the sum by c relative to
    sum |e_i x_i|: with A := sum(exp(-d_i) |x_i|) / S and Dx := sum(d_i exp(-d_i) |x_i|) / S, q := sx / se is off by
    err_q := A (c + 7 u + 2 a) + u Dx + |q| (theta + u);
  * H: err_lse + err_q + u |H|.
Each bound carries the factor 1.01 for the second-order terms of a first-order analysis.  Every quantity is computed in float64 from the INPUT row."""
import math

import numpy as np

U = 2.0 ** -24
NO_ID = -1


def scaled(row, temperature):
    """the finite mask and the float64 row the distribution is taken over"""
    row = np.asarray(row, dtype=np.float32)
    fin = np.isfinite(row)
    x = row.astype(np.float64)
    t = float(np.float32(temperature))
    if t != 0.0:
        x = x / t
    return fin, x


def restate(row, temperature, n):
    """(ids int64 [n], logprobs float64 [n], entropy float64) of one row"""
    fin, x = scaled(row, temperature)
    ids = np.full((n,), NO_ID, np.int64)
    lp = np.full((n,), -np.inf, np.float64)
    if not fin.any():
        return ids, lp, 0.0
    xf = np.where(fin, x, -np.inf)
    m = xf.max()
    e = np.where(fin, np.exp(xf - m), 0.0)
    se = e.sum()
    lse = m + math.log(se)
    h = lse - float((e[fin] * x[fin]).sum()) / se
    order = np.argsort(-xf, kind="stable")[:n]          # stable: a tie keeps the lower id
    k = int(min(n, fin.sum()))
    ids[:k] = order[:k]
    lp[:k] = xf[order[:k]] - lse
    return ids, lp, h


def bounds(row, temperature, n):
    """(bound of every log-probability [n] (inf where the pair is padding), bound of the entropy) of one row, float64"""
    fin, x = scaled(row, temperature)
    if not fin.any():
        return np.full((n,), np.inf), 0.0
    x = x[fin]
    V = len(np.asarray(row))
    m = x.max()
    d = m - x
    e = np.exp(-d)
    S = e.sum()
    a = 2 * U * float(np.abs(x).max()) if float(np.float32(temperature)) != 0.0 else 0.0
    c = (math.ceil(V / 1024) - 1 + 6 + 16) * U
    theta = c + 4 * U + 2 * a + U * float((d * e).sum()) / S
    lse = m + math.log(S)
    err_lse = a + theta + 4 * U * abs(math.log(S)) + U * abs(lse)
    q = float((e * x).sum()) / S
    A = float((e * np.abs(x)).sum()) / S
    Dx = float((d * e * np.abs(x)).sum()) / S
    err_q = A * (c + 7 * U + 2 * a) + U * Dx + abs(q) * (theta + U)
    h = lse - q
    top = np.sort(x)[::-1][:n] - lse
    blp = np.full((n,), np.inf)
    blp[:len(top)] = 1.01 * (err_lse + a + U * np.abs(top))
    return blp, 1.01 * (err_lse + err_q + U * abs(h))


# ---- rows of the kernel-alone test.  A thread of the 1024-thread sampler holds the ids tid, tid + 1024, ... ("its column"); wave w holds tid 64 w .. 64 w + 63
def random_rows(n_rows, V, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n_rows, V)) * 3.0).astype(np.float32)


def tie_rows(V, seed):
    """name -> row with exact ties among its largest entries, placed by where the sampler holds them"""
    base = random_rows(1, V, seed)[0]
    top = np.float32(np.abs(base).max() + 1.0)
    out = {}

    def put(name, ids, values):
        r = base.copy()
        for i, v in zip(ids, values):
            r[i] = v
        out[name] = r
    put("one thread's column", [5, 5 + 1024, 5 + 7 * 1024], [top, top, top])
    put("two threads of one wave", [70, 100, 70 + 1024], [top, top, top - np.float32(0.5)])
    put("two waves", [3 * 64 + 1, 9 * 64 + 2, 15 * 64 + 63], [top, top, top])
    put("the last id and id 0", [V - 1, 0], [top, top])
    put("ties below the best", [40000, 17, 30000, 18], [top, top - np.float32(1.0), top - np.float32(1.0), top - np.float32(1.0)])
    r = np.full((V,), -np.inf, np.float32)
    r[[V - 1, 1500, 23]] = [1.5, -2.0, 1.5]
    out["three finite entries"] = r
    r = np.full((V,), -np.inf, np.float32)
    r[777] = -3.25
    out["one finite entry"] = r
    return out
