"""Instruction-for-instruction comparison of the GPU kernels of two builds (the objects under <pkg>/build/ of two trees).

    python tools/isa_diff.py OLD_BUILD_DIR NEW_BUILD_DIR [-v] [--rename OLD=NEW ...]

For every .o of either directory: the gfx950 code object (kernel_resources.code_object), `llvm-objdump -d`, split by
kernel symbol, demangled.  Kernels are matched by demangled name over the whole build (which object holds a kernel, and in
which order, is not compared), after one normalisation: a trailing `, false` / `, true` template argument of
solve_kernel<...> that only the OLD build has (the retired PLDS parameter) is dropped.  --rename OLD=NEW pairs a kernel whose
name changed: the one kernel of the old build whose demangled name contains OLD with the one of the new build whose name
contains NEW (a kernel that became a template: --rename 'vsmpc::record_kernel(=vsmpc::record_kernel<false>(').  The s_nop
padding behind a kernel's last s_endpgm, up to the next symbol's alignment, is no instruction of the kernel and is dropped:
a template instantiation lies in a section of its own and has none.

Compared per kernel: the instruction text (mnemonic and operands; encodings and addresses are not; branch operands are
PC-relative and so position independent as they stand; the literal of a PC-relative address -- s_getpc_b64 followed by
s_add_u32 -- is replaced by the data object or the kernel it points into and the offset inside it -- a long branch inside
a kernel, so that a kernel does not differ because another kernel in front of it in the same object changed size -- or by
section and section offset where no symbol covers the address: where the constant tables lie relative to the code, and
behind how many kernel descriptors in .rodata, is layout; which table an instruction reads is not) and the resource notes of the
code-object metadata.

NOT compared: the constant data the kernels read (the tile tables and the kernel descriptors in .rodata).  A change that
alters a table's CONTENTS and no instruction passes here: compare .rodata of the code objects beside it when a refactor
touches the tables.

Prints one line per kernel (name, instruction count, same / DIFFERENT / missing) and exits non-zero on any difference, on
a kernel missing on either side, or when no kernel was found.  -v prints a unified diff of the first kernels that differ."""
from __future__ import annotations

import difflib
import glob
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import LLVM, code_object  # noqa: E402

NOTES = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
         "group_segment_fixed_size")
_SYM = re.compile(r"^[0-9a-f]+ <([^>]+)>:\s*$")
_INS = re.compile(r"^\s+(\S.*?)\s*//\s*([0-9A-Fa-f]+):")
_GETPC = re.compile(r"^s_getpc_b64 s\[(\d+):\d+\]")
_PCADD = re.compile(r"^(s_add_u32 s(\d+), s(\d+), )(0x[0-9a-f]+|-?\d+)$")
_SECTION = re.compile(r"^\s*\d+\s+(\S+)\s+([0-9a-f]+)\s+([0-9a-f]+)\s")
_OBJECT = re.compile(r"^([0-9a-f]+)\s+\S+\s+[OF]\s+\S+\s+([0-9a-f]+)\s+(?:\.\S+\s+)?(\S+)\s*$")


def demangle(names):
    names = list(names)
    if not names:
        return {}
    out = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def kernels_of(obj: str) -> dict:
    """{mangled kernel symbol: (instruction list, resource notes)} of one host object"""
    with tempfile.TemporaryDirectory() as tmp:
        co = os.path.join(tmp, "co")
        if not code_object(obj, co):
            return {}
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True).stdout
        dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], capture_output=True, text=True).stdout
        hdr = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-h", co], capture_output=True, text=True).stdout
        syms = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-t", co], capture_output=True, text=True).stdout
    sections = [(m.group(1), int(m.group(3), 16), int(m.group(2), 16)) for m in map(_SECTION.match, hdr.split("\n")) if m]

    objects = [(m.group(3), int(m.group(1), 16), int(m.group(2), 16)) for m in map(_OBJECT.match, syms.split("\n")) if m]

    def located(addr):
        for name, start, size in objects:
            if size and start <= addr < start + size:
                return f"<{name}+0x{addr - start:x}>"
        for name, start, size in sections:
            if size and start <= addr < start + size:
                return f"<{name}+0x{addr - start:x}>"
        return f"<0x{addr:x}>"
    res = {}
    for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        block = ".agpr_count:" + block
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            res[name.group(1)] = tuple(int(m.group(1)) if (m := re.search(rf"\.{f}:\s+(\d+)", block)) else -1 for f in NOTES)
    out, sym, getpc = {}, None, None
    for line in dis.split("\n"):
        m = _SYM.match(line)
        if m:
            sym = m.group(1)
            if sym in res:
                out[sym] = ([], res[sym])
            continue
        m = _INS.match(line)
        if m and sym in out:
            text = re.sub(r"\s+", " ", m.group(1))
            add = _PCADD.match(text)
            if getpc is not None and add and add.group(2) == add.group(3) == getpc:   # s_getpc_b64 yields this instruction's address
                lit = int(add.group(4), 0)
                text = add.group(1) + located(int(m.group(2), 16) + (lit - (1 << 32) if lit >= 1 << 31 else lit))
            pc = _GETPC.match(text)
            getpc = pc.group(1) if pc else None
            out[sym][0].append(text)
    return out


def build_kernels(build_dir: str) -> dict:
    """{demangled name: (instructions, notes, object)} over all objects of a build directory"""
    out = {}
    for obj in sorted(glob.glob(os.path.join(build_dir, "*.o"))):
        ks = kernels_of(obj)
        dem = demangle(ks)
        for sym, (ins, notes) in ks.items():
            name = dem.get(sym, sym)
            if name in out:
                raise SystemExit(f"kernel {name} appears twice in {build_dir} ({out[name][2]}, {os.path.basename(obj)})")
            while len(ins) > 1 and ins[-1].startswith("s_nop") and any(i.startswith("s_endpgm") for i in ins):
                ins.pop()
            out[name] = (ins, notes, os.path.basename(obj))
    return out


def main(argv) -> int:
    verbose = "-v" in argv
    renames = [argv[i + 1].split("=", 1) for i, a in enumerate(argv[:-1]) if a == "--rename"]
    dirs = [a for i, a in enumerate(argv) if a not in ("-v", "--rename") and (i == 0 or argv[i - 1] != "--rename")]
    if len(dirs) != 2:
        print(__doc__)
        return 2
    old, new = build_kernels(dirs[0]), build_kernels(dirs[1])
    for name in list(old):   # the retired PLDS argument: a last `, false` / `, true` the old name has and the new one lacks
        short = re.sub(r"(solve_kernel<.*), (?:false|true)>\(", r"\1>(", name)
        if short != name and name not in new and short in new and short not in old:
            old[short] = old.pop(name)
    if not old or not new:
        print("no kernels found")
        return 1
    for a, b in renames:
        olds, news = [n for n in old if a in n], [n for n in new if b in n]
        if len(olds) != 1 or len(news) != 1:
            print(f"--rename {a}={b}: {len(olds)} kernels of the old build and {len(news)} of the new one match")
            return 2
        print(f"renamed: {olds[0]} -> {news[0]}")
        old[news[0]] = old.pop(olds[0])
    bad, shown = 0, 0
    print("kernel | object | instructions | " + " ".join(n.replace("_count", "").replace("_fixed_size", "") for n in NOTES)
          + " | verdict")
    for name in sorted(set(old) | set(new)):
        short = name.replace("vsmpc::", "")
        short = short[:short.index("(")] if "(" in short else short
        if name not in old or name not in new:
            print(f"{short} | {(old.get(name) or new.get(name))[2]} | - | - | MISSING in {'old' if name not in old else 'new'} build")
            bad += 1
            continue
        (io, no, _), (inn, nn, on) = old[name], new[name]
        same_i, same_n = io == inn, no == nn
        notes = " ".join(str(v) for v in nn) if same_n else " ".join(f"{a}->{b}" for a, b in zip(no, nn))
        count = str(len(inn)) if len(io) == len(inn) else f"{len(io)}->{len(inn)}"
        verdict = "same" if same_i and same_n else ("DIFFERENT" + ("" if same_i else " instructions") + ("" if same_n else " notes"))
        print(f"{short} | {on} | {count} | {notes} | {verdict}")
        if not (same_i and same_n):
            bad += 1
            if verbose and not same_i and shown < 3:
                shown += 1
                print("\n".join(list(difflib.unified_diff(io, inn, "old", "new", lineterm="", n=2))[:200]))
    print(f"{len(set(old) | set(new))} kernels, {bad} differ or are missing")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
