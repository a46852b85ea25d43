"""tools/device_code_hash.py on canned disassembly: --instructions-only compares builds whose kernels were renamed (trailing padding dropped, hashes
alone), the default per-name output is what it has always been.  No GPU, no toolchain: function_hashes / report take the disassembler's text."""
import hashlib
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("device_code_hash", os.path.join(ROOT, "tools", "device_code_hash.py"))
H = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(H)

HEAD = "\nbundle.co:\tfile format elf64-amdgpu\n\nDisassembly of section .text:\n\n"
FILL = ["\ts_load_dwordx2 s[0:1], s[4:5], 0x0", "\ts_waitcnt lgkmcnt(0)", "\tv_mov_b32_e32 v0, 0                            // 000000001008: 7E000280", "\tglobal_store_dword v0, v0, s[0:1]",
        "\ts_nop 0", "\ts_endpgm"]      # (an s_nop 0 INSIDE a function is an instruction like any other)
SCALE = ["\ts_load_dwordx4 s[0:3], s[4:5], 0x0", "\tv_lshlrev_b32_e32 v0, 2, v0", "\ts_waitcnt lgkmcnt(0)", "\tglobal_load_dword v1, v0, s[0:1]", "\ts_waitcnt vmcnt(0)",
         "\tv_mul_f32_e32 v1, s2, v1", "\tglobal_store_dword v0, v1, s[0:1]", "\ts_endpgm"]


def text(functions):
    """functions: (name, instruction lines, padding lines) in the order of the code object"""
    return HEAD + "".join(f"<{name}>:\n" + "\n".join(body + pad) + "\n\n" for name, body, pad in functions)


# the same two instruction sequences: plain functions padded with s_nop 0 up to the next one, and - renamed, the other way round - template instantiations, whose
# padding the disassembler prints as `...`; the last function of a code object ends in s_code_end
OLD = text([("_ZN2wh11fill_kernelEPf", FILL, ["\ts_nop 0"] * 5), ("_ZN2wh12scale_kernelEPff", SCALE, ["\ts_code_end"] * 3)])
NEW = text([("_ZN2wh12scale_kernelILNS_4ModeE1EEEvPff", SCALE, ["\t..."]), ("_ZN2wh11fill_kernelILNS_4ModeE0EEEvPf", FILL, ["\ts_nop 0", "\ts_code_end", "\ts_code_end"])])


def lines(disassembly, instructions_only):
    return H.report(H.function_hashes(disassembly, instructions_only), instructions_only)


def test_instructions_only_is_equal_for_renamed_reordered_and_differently_padded_functions():
    old, new = lines(OLD, True), lines(NEW, True)
    assert old == new and len(old) == 2 and len(set(old)) == 2
    assert all(len(h) == 40 and " " not in h for h in old) and old == sorted(old)      # the hashes alone, sorted: no names
    assert lines(OLD, False) != lines(NEW, False)                                       # (the default output tells the two apart)


def test_instructions_only_differs_once_one_instruction_differs():
    changed = NEW.replace("v_mul_f32_e32 v1, s2, v1", "v_mul_f32_e32 v1, s3, v1")
    assert changed != NEW
    old, new = lines(OLD, True), lines(changed, True)
    assert old != new and len(set(old) & set(new)) == 1      # the untouched function still matches
    # a trailing s_nop 0 is padding, one in front of the last instruction is not
    moved = text([("f", FILL[:4] + FILL[5:], ["\ts_nop 0"])])
    assert lines(moved, True) != lines(text([("f", FILL, [])]), True)


def test_default_output_is_the_per_name_hash_of_every_line_behind_the_label():
    def sha(rows):      # the tool as it was: every non-blank line, comment stripped, one per line
        return hashlib.sha1("".join(r + "\n" for r in rows).encode()).hexdigest()
    fill = ["s_load_dwordx2 s[0:1], s[4:5], 0x0", "s_waitcnt lgkmcnt(0)", "v_mov_b32_e32 v0, 0", "global_store_dword v0, v0, s[0:1]", "s_nop 0", "s_endpgm"]
    unpadded = text([("_ZN2wh11fill_kernelEPf", FILL, [])])
    assert lines(unpadded, False) == ["_ZN2wh11fill_kernelEPf " + sha(fill)]
    assert lines(unpadded, True) == [sha(fill)]                                   # nothing to drop: the same hash, without the name
    # the default keeps hashing the padding, sorted by name
    got = lines(OLD, False)
    assert got == ["_ZN2wh11fill_kernelEPf " + sha(fill + ["s_nop 0"] * 5), "_ZN2wh12scale_kernelEPff " + sha([r.strip() for r in SCALE] + ["s_code_end"] * 3)]
