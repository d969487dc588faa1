#!/usr/bin/env python3
"""Per-kernel comparison of two builds of libsegengine.so (CPU only; needs llvm-objdump and llvm-readelf; llvm-cxxfilt or c++filt for readable names).

    python scripts/kernel_diff.py [--by-name] OLD/libsegengine.so NEW/libsegengine.so

Extracts the gfx950 code objects of both libraries (one per translation unit, in link order), lists their kernels - the functions
that have a 64-byte kernel descriptor `<name>.kd` - and for every kernel present in both compares the code and the descriptor.
Prints the removed kernels, the added kernels and every kernel whose code differs; exit status 1 if any code differs.

Two things move with the layout of a code object and say nothing about a kernel's code:
  * the descriptor's code-entry offset (bytes 16 - 23): masked;
  * the literal of a pc-relative address of a device global (e.g. an arrival counter): where the bytes of a kernel differ, both
    versions are disassembled and must agree line by line except for single numeric literals, and each such literal must have
    changed by exactly the change of the distance between the kernel and ONE data object both code objects define.
--by-name pairs the kernels by their demangled name with the namespace qualifiers removed instead of by their symbol: for a change
that moves kernels, or the types in their signatures, into another namespace or another translation unit.  A kernel that several
translation units define is numbered in link order among its namesakes; two different symbols of one library that collapse onto
one name are an error (exit status 2).
The script compares; it does not look for any particular instruction.  Objects in .bss have no file bytes and are not compared."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")


def tool(name):
    p = os.path.join(LLVM, name)
    return p if os.path.exists(p) else (shutil.which(name) or name)


def run(*cmd, cwd=None):
    return subprocess.run(cmd, cwd=cwd, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout


class CodeObject:
    def __init__(self, path):
        self.path = path
        self.data = open(path, "rb").read()
        self.sections = {}   # index -> (name, type, addr, offset, size)
        for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+(\S+)\s+(\S+)\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", run(tool("llvm-readelf"), "-SW", path), re.M):
            self.sections[int(m.group(1))] = (m.group(2), m.group(3), int(m.group(4), 16), int(m.group(5), 16), int(m.group(6), 16))
        self.funcs, self.objects = {}, {}   # name -> (addr, size, section index)
        for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+(FUNC|OBJECT)\s+\S+\s+\S+\s+(\d+)\s+(\S+)$", run(tool("llvm-readelf"), "-sW", path), re.M):
            (self.funcs if m.group(3) == "FUNC" else self.objects)[m.group(5)] = (int(m.group(1), 16), int(m.group(2)), int(m.group(4)))
        self.kernels = sorted(n for n in self.funcs if n + ".kd" in self.objects)

    def bytes_of(self, sym):
        addr, size, ndx = sym
        _, typ, saddr, soff, _ = self.sections[ndx]
        if typ == "NOBITS":
            return None
        return self.data[soff + addr - saddr: soff + addr - saddr + size]

    def descriptor(self, k):
        b = bytearray(self.bytes_of(self.objects[k + ".kd"]))
        b[16:24] = bytes(8)   # KERNEL_CODE_ENTRY_BYTE_OFFSET: descriptor -> code, moves with the layout
        return bytes(b)

    def disassembly(self, k):
        out = run(tool("llvm-objdump"), "-d", "--no-leading-addr", "--no-show-raw-insn", "--disassemble-symbols=" + k, self.path)
        lines = [ln.split("//")[0].strip() for ln in out.splitlines()]
        return [ln for ln in lines if ln and not ln.endswith(":") and not ln.startswith(("Disassembly", self.path))]


def code_objects(lib, tmp):
    d = tempfile.mkdtemp(dir=tmp)
    local = os.path.join(d, "lib.so")
    shutil.copy(lib, local)
    run(tool("llvm-objdump"), "--offloading", "lib.so", cwd=d)
    names = [f for f in os.listdir(d) if f.endswith("gfx950") and os.path.getsize(os.path.join(d, f)) > 0]
    names.sort(key=lambda f: int(f.split(".")[2]))
    return [CodeObject(os.path.join(d, f)) for f in names]


QUALIFIER = re.compile(r"(?:\(anonymous namespace\)|\b[A-Za-z_]\w*)::")
NUM = re.compile(r"(?<![\w.])(-?(?:0x[0-9a-fA-F]+|\d+))(?![\w.])")


def data_objects(co, by_name):
    """name -> address of the data objects a code object defines (with by_name: demangled, namespace qualifiers removed)."""
    names = [o for o in co.objects if not o.endswith(".kd")]
    keys = [QUALIFIER.sub("", d) for d in demangle(names)] if by_name else names
    return {key: co.objects[o][0] for key, o in zip(keys, names)}


def literal_moves(old, new, k, kn, by_name=False):
    """Both disassemblies (of `k` in old, `kn` in new) agree except for literals that moved with the layout: the number of such literals, or None."""
    a, b = old.disassembly(k), new.disassembly(kn)
    if len(a) != len(b):
        return None
    shift = new.funcs[kn][0] - old.funcs[k][0]
    od, nd = data_objects(old, by_name), data_objects(new, by_name)
    allowed = {nd[o] - od[o] - shift for o in od if o in nd}
    moved = 0
    for x, y in zip(a, b):
        if x == y:
            continue
        if NUM.sub("#", x) != NUM.sub("#", y):
            return None
        diff = [(int(p, 0), int(q, 0)) for p, q in zip(NUM.findall(x), NUM.findall(y)) if p != q]
        if len(diff) != 1 or (diff[0][1] - diff[0][0]) not in allowed:
            return None
        moved += 1
    return moved


def kernel_table(objs):
    """kernel key -> (code object, name); a name defined by more than one translation unit gets the unit's index appended."""
    seen, table = {}, {}
    for i, co in enumerate(objs):
        for k in co.kernels:
            seen[k] = seen.get(k, 0) + 1
    for i, co in enumerate(objs):
        for k in co.kernels:
            table[k if seen[k] == 1 else f"{k}@unit{i}"] = (co, k)
    return table


def kernel_table_by_name(objs):
    """demangled name without namespace qualifiers -> (code object, symbol); namesakes of several units are numbered in link order."""
    syms = sorted({k for co in objs for k in co.kernels})
    plain = {k: QUALIFIER.sub("", d) for k, d in zip(syms, demangle(syms))}
    owner = {}
    for k, name in plain.items():
        if owner.setdefault(name, k) != k:
            sys.exit(f"kernel_diff: two kernels collapse onto one name without namespaces: {name}\n    {owner[name]}\n    {k}")
    count = {k: sum(k in co.kernels for co in objs) for k in syms}
    seen, table = {}, {}
    for co in objs:
        for k in co.kernels:
            n = seen.get(k, 0)
            seen[k] = n + 1
            table[plain[k] if count[k] == 1 else f"{plain[k]} #{n}"] = (co, k)
    return table


def demangle(names):
    if not names:
        return []
    filt = next((t for t in (tool("llvm-cxxfilt"), "c++filt") if shutil.which(t)), None)
    if filt is None:
        return list(names)
    # (older demanglers do not know DF16b, the bf16 type: it goes in as `half`, a builtin type the library never uses, and comes out renamed)
    out = subprocess.run([filt], input="\n".join(n.split("@unit")[0].replace("DF16b", "Dh") for n in names), stdout=subprocess.PIPE, text=True, check=True).stdout
    return [re.sub(r"\b(half|_Float16|__fp16)\b", "bf16", d).replace("(anonymous namespace)::", "") for d in out.splitlines()]


def main():
    by_name = "--by-name" in sys.argv[1:]
    args = [a for a in sys.argv[1:] if a != "--by-name"]
    if len(args) != 2:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        old_objs, new_objs = code_objects(args[0], tmp), code_objects(args[1], tmp)
        table = kernel_table_by_name if by_name else kernel_table
        old, new = table(old_objs), table(new_objs)
        show = (lambda keys: list(keys)) if by_name else demangle
        removed, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
        same = moved = 0
        differs = []
        for key in sorted(set(old) & set(new)):
            (oc, k), (nc, kn) = old[key], new[key]   # (the symbols differ only with --by-name)
            if oc.descriptor(k) != nc.descriptor(kn):
                differs.append((key, "kernel descriptor"))
            elif oc.bytes_of(oc.funcs[k]) == nc.bytes_of(nc.funcs[kn]):
                same += 1
            else:
                n = literal_moves(oc, nc, k, kn, by_name)
                if n is None:
                    differs.append((key, "instruction stream"))
                else:
                    moved += 1

        def text_bytes(objs):
            return sum(s[4] for co in objs for s in co.sections.values() if s[0] == ".text")
        print(f"old: {len(old_objs)} code objects, {len(old)} kernels, {text_bytes(old_objs)} bytes of .text, library {os.path.getsize(args[0])} bytes")
        print(f"new: {len(new_objs)} code objects, {len(new)} kernels, {text_bytes(new_objs)} bytes of .text, library {os.path.getsize(args[1])} bytes")
        for i, (a, b) in enumerate(zip(old_objs, new_objs)):
            if len(a.kernels) != len(b.kernels):
                print(f"  code object {i}: {len(a.kernels)} -> {len(b.kernels)} kernels, {len(a.data)} -> {len(b.data)} bytes")
        print(f"kernels in both: {same + moved + len(differs)}")
        print(f"  identical code bytes and descriptor: {same}")
        print(f"  identical instructions, only address literals of device globals moved with the layout: {moved}")
        print(f"  DIFFERENT: {len(differs)}")
        for key, what in differs:
            print(f"    {what}: {show([key])[0]}")
        print(f"added kernels: {len(added)}")
        for d in show(added):
            print(f"    {d}")
        print(f"removed kernels: {len(removed)}")
        for d in show(removed):
            print(f"    {d}")
        return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main())
