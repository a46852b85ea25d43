#!/usr/bin/env python3
"""What does the split-precision encoder (encoder_precision 1) buy end to end?  CPU oracle prediction, no GPU.

Restates the oracle encoder (oracle/model.py OracleWhisper.encode, as tests/tools/encoder_error_attribution.py does) with every rounding
point of the device modelled, and reports each variant's end-to-end logits error against the all-fp32 oracle, divided by the logits'
standard deviation:

    device now   Float16 at mel, GELU(conv1), both LayerNorm outputs, q / k / v / P, the attention output, GELU(fc1) and the output
    floor        fp32 everywhere, the output rounded once to Float16 (the reference's AudioEncoderOutput type)
    split        hi | lo pairs (hilo below) at mel, GELU(conv1), both LayerNorm outputs, the attention output, GELU(fc1) and the output;
                 q / k / v / P stay Float16 - what csrc/ computes for a split session
    split, f16 self cache   the same, decoded with the Float16 self-attention cache the device keeps

The split rows are the prediction tests/test_gpu_split_encoder.py checks on the device.  Usage:

    python tests/tools/split_encoder_prediction.py [--models large-v3,small,tiny.en] [--out profiles/r07_split_encoder_prediction.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import decode as OD  # noqa: E402
from oracle import mel as omel  # noqa: E402
from oracle.model import OracleWhisper  # noqa: E402
from realistic import realistic_state_dict  # noqa: E402
from whisperkit_amd import weights  # noqa: E402
from whisperkit_amd.synth import synthetic_chunk  # noqa: E402


def hilo(x):
    """The value a hi | lo Float16 pair carries: hi = f16(x), lo = f16(x - hi) (x - hi is exact in fp32; Float16 subnormals included) -
    csrc/kernels.h split_f16.  Accepts a numpy array or a torch tensor (fp32)."""
    if isinstance(x, np.ndarray):
        x = np.asarray(x, np.float32)
        hi = x.astype(np.float16).astype(np.float32)
        return hi + (x - hi).astype(np.float16).astype(np.float32)
    hi = x.half().float()
    return hi + (x - hi).half().float()


def f16(x):
    return x.half().float()


def fp32(x):
    return x


def encode(om, mel, at_operands, at_qkvp, at_output):
    """OracleWhisper.encode with `at_operands` applied at the GEMM operands (mel, GELU(conv1), LayerNorm outputs, attention output,
    GELU(fc1)), `at_qkvp` at q / k / v / P and `at_output` at the encoder output; each one of f16 / hilo / fp32"""
    w, dims = om.w, om.dims
    H = dims.n_audio_head
    with torch.no_grad():
        x = at_operands(torch.from_numpy(np.ascontiguousarray(mel, dtype=np.float32)))[None]
        x = at_operands(F.gelu(F.conv1d(x, w["encoder.conv1.weight"], w["encoder.conv1.bias"], padding=1)))
        x = F.gelu(F.conv1d(x, w["encoder.conv2.weight"], w["encoder.conv2.bias"], stride=2, padding=1))
        x = x[0].T + w["encoder.positional_embedding"]
        T, d = x.shape
        hd = d // H
        for i in range(dims.n_audio_layer):
            p = f"encoder.blocks.{i}"
            xn = at_operands(F.layer_norm(x, (d,), w[p + ".attn_ln.weight"], w[p + ".attn_ln.bias"]))
            q = at_qkvp(F.linear(xn, w[p + ".attn.query.weight"], w[p + ".attn.query.bias"]) * hd ** -0.5)
            k = at_qkvp(F.linear(xn, w[p + ".attn.key.weight"]))
            v = at_qkvp(F.linear(xn, w[p + ".attn.value.weight"], w[p + ".attn.value.bias"]))
            qh, kh, vh = (t.view(T, H, hd).permute(1, 0, 2) for t in (q, k, v))
            s = qh @ kh.transpose(1, 2)
            e = at_qkvp(torch.exp(s - s.max(dim=-1, keepdim=True).values))
            o = (e @ vh) / e.sum(dim=-1, keepdim=True)
            o = at_operands(o.permute(1, 0, 2).reshape(T, d))
            x = x + F.linear(o, w[p + ".attn.out.weight"], w[p + ".attn.out.bias"])
            xn = at_operands(F.layer_norm(x, (d,), w[p + ".mlp_ln.weight"], w[p + ".mlp_ln.bias"]))
            h = at_operands(F.gelu(F.linear(xn, w[p + ".mlp.0.weight"], w[p + ".mlp.0.bias"])))
            x = x + F.linear(h, w[p + ".mlp.2.weight"], w[p + ".mlp.2.bias"])
        x = at_output(F.layer_norm(x, (d,), w["encoder.ln_post.weight"], w["encoder.ln_post.bias"]))
    return x.numpy()


def predict(model, tokens, seed):
    dims = weights.MODEL_DIMS[model]
    om = OracleWhisper(dims, realistic_state_dict(dims, seed=0))
    st, langs = OD.special_tokens_for_vocab(dims.n_vocab)
    mel = omel.log_mel_spectrogram(synthetic_chunk(seed), dims.n_mels).astype(np.float32)
    t0 = time.time()
    ref_enc = encode(om, mel, fp32, fp32, fp32)
    assert np.abs(ref_enc - om.encode(mel)).max() < 1e-4 * max(1.0, float(np.abs(ref_enc).max())), "the restated encoder must be the oracle's"
    kw = dict(firstTokenLogProbThreshold=None, logProbThreshold=None, compressionRatioThreshold=None, temperatureFallbackCount=0, sampleLength=tokens)
    oopts = OD.DecodingOptions(**kw)
    state = om.new_state(ref_enc)
    ores = OD.decode_text(lambda t, p: state.step(t, p, want_alignment=False), OD.prefill_prompt(oopts, st, dims.is_multilingual),
                          OD.GreedyTokenSampler(0.0, st.endToken, oopts), oopts, st, dims.is_multilingual, langs)
    inputs = ores.tokens[:-1][: tokens - 1]
    n = len(inputs)
    full = om.new_state(ref_enc).forward_full(inputs, want_alignment=False)
    sigma = float(np.std(np.stack([full[p] for p in range(0, n, 8)])))
    rms = float(np.sqrt((ref_enc ** 2).mean()))

    def logits_err(enc, kv16=False):
        got = om.new_state(enc, kvFloat16=kv16, crossFloat16=False).forward_full(inputs, want_alignment=False)
        return max(float(np.abs(got[p] - full[p]).max()) for p in range(n)) / sigma

    def enc_err(enc):
        e = np.abs(enc - ref_enc)
        return {"encoder_max_abs_err": float(e.max()), "encoder_rms_err_over_rms": float(np.sqrt((e ** 2).mean())) / rms}

    rows = {}
    now = encode(om, mel, f16, f16, f16)
    rows["device now: Float16 operands, q / k / v / P and output"] = {"logits_rel_sigma": logits_err(now), **enc_err(now)}
    floor = ref_enc.astype(np.float16).astype(np.float32)
    rows["floor: fp32, output rounded to Float16"] = {"logits_rel_sigma": logits_err(floor), **enc_err(floor)}
    split = encode(om, mel, hilo, f16, hilo)
    rows["split: hi | lo operands and output, q / k / v / P Float16"] = {"logits_rel_sigma": logits_err(split), **enc_err(split)}
    rows["split, decoder with the Float16 self-attention cache"] = {"logits_rel_sigma": logits_err(split, kv16=True), **enc_err(split)}
    print(f"{model}: {n} decoder inputs, sigma {sigma:.2f}: " + ", ".join(f"{k.split(':')[0]} {v['logits_rel_sigma']:.2e}" for k, v in rows.items())
          + f" [{time.time() - t0:.0f} s]", flush=True)
    return {"weights": "tests/realistic.py realistic_state_dict(seed 0)", "chunk_seed": seed, "decoder_inputs": n, "logits_sigma": sigma,
            "encoder_output_rms": rms, "variants": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="large-v3,small,tiny.en")
    ap.add_argument("--tokens", type=int, default=96)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_split_encoder_prediction.json"))
    args = ap.parse_args()
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    doc = {"note": "oracle only (torch fp32 on the CPU); logits errors are max |delta| over all decoder positions / sigma(logits) against the "
                   "all-fp32 oracle on the fp32 oracle's own greedy inputs", "models": {}}
    for m in args.models.split(","):
        doc["models"][m] = predict(m, args.tokens, args.seed)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
