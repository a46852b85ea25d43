#!/usr/bin/env python3
"""Per-kernel hash of the gfx950 device code of a built library: unbundles every code object of the .hip_fatbin section, disassembles it and
prints `<mangled kernel> <sha1 of its instructions>` per function (sorted).  Two builds with the same flags hold the same kernels with the
same instructions exactly when the outputs are equal:
    python tools/device_code_hash.py parent/whisperkit_amd/libwhisperhip.so > a.txt
    python tools/device_code_hash.py whisperkit_amd/libwhisperhip.so > b.txt && diff a.txt b.txt
--instructions-only compares builds whose kernels were renamed (a function that became a template instantiation, a changed parameter type): per
function the alignment padding behind the last instruction is dropped (it differs with the symbol's kind), and the hashes are printed alone,
sorted.  The outputs are equal exactly when the two builds hold the same multiset of instruction sequences:
    python tools/device_code_hash.py --instructions-only parent/whisperkit_amd/libwhisperhip.so > a.txt   (and so on)"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
PADDING = ("s_nop 0", "s_code_end", "...")      # what follows a function's last instruction up to the next function's alignment


def function_hashes(disassembly, instructions_only=False):
    """(mangled name, sha1 of its lines) per function of one code object's `llvm-objdump -d --no-show-raw-insn --no-leading-addr` text, in the
    text's order.  Comments and blank lines are no part of a hash; with instructions_only neither is the trailing padding."""
    functions = []
    for line in disassembly.splitlines():
        m = re.match(r"^<([^>]+)>:\s*$", line)
        if m:
            functions.append((m.group(1), []))
        elif functions and line.strip():
            functions[-1][1].append(re.sub(r"//.*$", "", line).strip())
    out = []
    for name, lines in functions:
        while instructions_only and lines and lines[-1] in PADDING:
            lines.pop()
        out.append((name, hashlib.sha1("".join(l + "\n" for l in lines).encode()).hexdigest()))
    return out


def report(hashes, instructions_only=False):
    """The lines main() prints for a list of (name, hash)."""
    if instructions_only:
        return sorted(h for _, h in hashes)
    return [f"{name} {h}" for name, h in sorted(hashes)]


def main(lib, instructions_only=False):
    hashes = []
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
            hashes += function_hashes(dis, instructions_only)
    names = [name for name, _ in hashes]
    assert len(set(names)) == len(names), sorted(n for n in set(names) if names.count(n) > 1)
    for line in report(hashes, instructions_only):
        print(line)
    print(f"{len(starts)} code objects, {len(hashes)} functions", file=sys.stderr)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--instructions-only"]
    main(args[0], instructions_only=len(args) != len(sys.argv) - 1)
