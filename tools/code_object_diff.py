#!/usr/bin/env python3
"""Diagnostic (not part of the product): compare the gfx950 kernels of two builds of the library.

    python tools/code_object_diff.py OLD.so NEW.so

Per kernel: the disassembly (no raw bytes, addresses and trailing comments stripped) and the note metadata that decides
how it runs (registers, spills, scratch, LDS, kernarg size).  Which code object of a build holds a kernel does not
matter.  Prints the kernels that are missing, added or different; exits non-zero if there are any.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
META = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size", "kernarg_segment_size")


def kernels(lib, tmp):
    """{kernel symbol: (disassembly text, {metadata key: value})} over every gfx950 code object of `lib`."""
    run = lambda *cmd: subprocess.run(cmd, check=True, capture_output=True, text=True, cwd=tmp).stdout
    shutil.copy(lib, tmp)
    run(f"{LLVM}/llvm-objdump", "--offloading", os.path.basename(lib))  # extracts the code objects next to the copy
    out = {}
    for f in sorted(os.listdir(tmp)):
        if "gfx950" not in f:
            continue
        meta = {}
        notes = run(f"{LLVM}/llvm-readelf", "--notes", f)
        for entry in re.split(r"\n(?=  - \.agpr_count:)", notes)[1:]:
            name = re.search(r"\n    \.name:\s+(\S+)", entry)
            if name:
                meta[name.group(1)] = {k: int(v) for k, v in re.findall(r"^[ -]{4}\.(\w+):\s+(\d+)[ \t]*$", entry, re.M)
                                       if k in META}
        # cut at the symbols; of an instruction line keep the text between its address and its trailing comment
        for sym, body in re.findall(r"^[0-9a-f]+ <([^>]+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)",
                                    run(f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", f), re.M | re.S):
            if sym in meta:
                lines = [re.sub(r"\s*//.*$", "", re.sub(r"^\s*[0-9a-f]+:\s*", "", l)).strip()
                         for l in body.splitlines() if l.strip()]
                while lines and lines[-1] in ("s_nop 0", "s_code_end", "..."):  # padding up to the next symbol
                    lines.pop()
                out[sym] = ("\n".join(lines), meta[sym])
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as t_old, tempfile.TemporaryDirectory() as t_new:
        old, new = kernels(sys.argv[1], t_old), kernels(sys.argv[2], t_new)
    bad = 0
    for k in sorted(set(old) | set(new)):
        what = []
        if k not in new or k not in old:
            what.append("missing" if k not in new else "added")
        else:
            if old[k][0] != new[k][0]:
                what.append(f"text differs ({old[k][0].count(chr(10)) + 1} -> {new[k][0].count(chr(10)) + 1} lines)")
            what += [f"{m}: {old[k][1].get(m)} -> {new[k][1].get(m)}" for m in META if old[k][1].get(m) != new[k][1].get(m)]
        if what:
            bad += 1
            print(k, "--", "; ".join(what))
    print(f"{len(old)} kernels in {sys.argv[1]}, {len(new)} in {sys.argv[2]}: {bad} missing, added or different")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
