#!/usr/bin/env python3
"""Per-kernel hash of the gfx950 device code of a built library: unbundles every code object of the .hip_fatbin section, disassembles it and
prints `<mangled kernel> <sha1 of its instructions>` per function (sorted).  Two builds with the same flags hold the same kernels with the
same instructions exactly when the outputs are equal:
    python tools/device_code_hash.py parent/whisperkit_amd/libwhisperhip.so > a.txt
    python tools/device_code_hash.py whisperkit_amd/libwhisperhip.so > b.txt && diff a.txt b.txt"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def main(lib):
    hashes = {}
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fatbin")
        subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", blob)]      # one bundle per translation unit
        for i, s in enumerate(starts):
            part, co = os.path.join(tmp, f"bundle{i}"), os.path.join(tmp, f"bundle{i}.co")
            open(part, "wb").write(blob[s:starts[i + 1] if i + 1 < len(starts) else len(blob)])
            subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=" + TARGET, "--input=" + part, "--output=" + co, "--unbundle"], check=True)
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co], check=True, capture_output=True, text=True).stdout
            cur = None
            for line in dis.splitlines():
                m = re.match(r"^<([^>]+)>:\s*$", line)
                if m:
                    cur = m.group(1)
                    assert cur not in hashes, cur
                    hashes[cur] = hashlib.sha1()
                elif cur and line.strip():
                    hashes[cur].update(re.sub(r"//.*$", "", line).strip().encode() + b"\n")
    for k in sorted(hashes):
        print(k, hashes[k].hexdigest())
    print(f"{len(starts)} code objects, {len(hashes)} functions", file=sys.stderr)


if __name__ == "__main__":
    main(sys.argv[1])
