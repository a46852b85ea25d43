#!/usr/bin/env python3
"""Decoder-step time of tiny.en (d = 384, 4 + 4 layers, synthetic weights) with the K / V rows (mode 0) and with the absorbed cross-attention
(mode 1), one lone session of 32 / 128 / 256 slots: a record for the later decision about the automatic mode at this width, not a gate.

    python tools/xabs_tiny_width_time.py [slots,slots,...] [modes]          (default 32,128,256 and 0,1)

Per cell: one warm-up decode (graph capture), then three timed decodes of 223 decoder steps each - a host clock around decodeText that ends in a
stream synchronise - and the per-kernel HIP-event averages of the cross-attention launches (wh_measure_kernels: dec_cross_attn is xabs_attn in
mode 1).  One JSON line per cell.  algorithmic_mb_per_layer_launch = the bytes the cross-attention of ONE layer has to move: mode 1
slots x 1500 x 384 x 2 (the Float16 encoder output) + Q' hi | lo + the partials; mode 0 slots x 2 x 1500 x 384 x 3 (24-bit K and V rows)."""
import ctypes, json, os, sys, threading, time
import numpy as np
if os.environ.get("WH_TOOL_NO_TORCH") != "1":
    import torch  # noqa: F401  (bench.py's process set-up: torch's HIP runtime is the one in the process; profiles/r03k_*)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from whisperkit_amd import api, weights
from whisperkit_amd.synth import synthetic_chunk

slots = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "32,128,256").split(",")]
modes = [int(x) for x in (sys.argv[2] if len(sys.argv) > 2 else "0,1").split(",")]
dims = weights.MODEL_DIMS["tiny.en"]
d, H, L_ = dims.n_text_state, dims.n_text_head, dims.n_text_layer
model = api.Model(dims, weights.synthetic_state_dict(dims, seed=0))
opts = api.DecodingOptions(firstTokenLogProbThreshold=None, logProbThreshold=None, compressionRatioThreshold=None,
                           noSpeechThreshold=None, temperatureFallbackCount=0)
def cell(B, mode):
    if True:
        s = api.Session(model, B, crossAttentionMode=mode)
        assert s.crossAttentionMode == mode
        for b in range(B):
            s.padOrTrim(synthetic_chunk(1234 + b), b)
        s.logMelSpectrogram(B); s.encodeFeatures(B); s.prepareDecoderInputs(B)
        prompt = s.prefillPrompt(opts)
        s.decodeText(prompt, opts, batch=B); s.synchronize()          # warm-up: graph capture, code objects
        runs, steps = [], 0
        for _ in range(3):
            s.prepareDecoderInputs(B); s.synchronize()
            a = time.perf_counter(); r = s.decodeText(prompt, opts, batch=B); s.synchronize()
            steps = r[0].steps
            runs.append((time.perf_counter() - a) * 1e3 / steps)
        splits = s.crossAttentionSplits
        if mode == 1:
            mb = (B * 1500 * d * 2 + 2 * B * 16 * d * 2 + splits * H * d * B * 4 + splits * H * B * 8) / 1e6
        else:
            mb = B * 2 * 1500 * d * 3 / 1e6
        lib = s.lib
        nk = lib.wh_kernel_kind_count()
        avg = (ctypes.c_double * nk)(); cnt = (ctypes.c_int32 * nk)()
        api._check(lib.wh_measure_kernels(s.handle, B, 16, avg, cnt))
        ks = {lib.wh_kernel_kind_name(k).decode(): round(avg[k], 2) for k in range(nk) if cnt[k]}
        ks = {k: v for k, v in ks.items() if k in ("dec_cross_attn", "dec_xabs_qk", "dec_xabs_vup")}
        rec = {"model": "tiny.en", "slots": B, "mode": mode, "key_splits": splits, "decoder_steps": steps,
               "ms_per_decoder_step_runs": [round(x, 4) for x in runs], "ms_per_decoder_step_median": round(float(np.median(runs)), 4),
               "cross_attention_kernels_us": ks, "algorithmic_mb_per_layer_launch": round(mb, 2)}
        if "dec_cross_attn" in ks:
            rec["cross_attn_tb_per_s"] = round(mb / ks["dec_cross_attn"], 3)          # MB / us = TB / s
        print(json.dumps(rec), flush=True)
        s.close()


for B in slots:
    for mode in modes:                      # the two modes of a size back to back
        th = threading.Thread(target=cell, args=(B, mode))          # graph capture on a worker thread, as bench.py does (under rocprofv3 a capture
        th.start(); th.join()                                       # on the main thread crashes inside the tool: profiles/r03j_*)
