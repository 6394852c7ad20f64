"""Compares the gfx950 machine code of two builds of liblitho_abbe.so kernel by kernel.

    python scripts/kernel_disasm_diff.py OLD.so NEW.so [name-regex] [OLDTYPE=NEWTYPE ...]

Extracts the device code object of each library, disassembles it (llvm-objdump -d) and compares the instruction
streams of the kernels both builds have (addresses and encodings dropped, branch targets kept as offsets into the
kernel).  Prints the kernels that differ, the ones only one build has, and a one-line summary; exit status 1 when a
common kernel matching the regex differs.  Used to show that a change which adds kernels (weighted x-pass siblings)
leaves the existing ones bit-identical.  Kernels are paired by their full signature; OLDTYPE=NEWTYPE rewrites a type name in the
old build's signatures first, for a change that renames the type of a kernel argument and nothing else about the kernel."""
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
LLVM = os.path.join(ROCM, "llvm", "bin")


MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(lib, tmp):
    """The gfx950 code objects of the library: its .hip_fatbin section holds one offload bundle per translation unit."""
    fat = os.path.join(tmp, "fat.bin")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
    data = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(MAGIC, data)] + [len(data)]
    out = []
    for i, (a, b) in enumerate(zip(starts, starts[1:])):
        bundle, co = os.path.join(tmp, f"b{i}.bundle"), os.path.join(tmp, f"b{i}.co")
        open(bundle, "wb").write(data[a:b])
        targets = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--list", "--type=o", f"--input={bundle}"],
                                 capture_output=True, text=True, check=True).stdout.split()
        for t in targets:
            if "gfx950" in t:
                subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={bundle}",
                                f"--targets={t}", f"--output={co}"], check=True)
                out.append(co)
    return out


def kernels(cos):
    table, name, pcrel = {}, None, 0
    text = "\n".join(subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "-C", co], capture_output=True,
                                    text=True, check=True).stdout for co in cos)
    for line in text.splitlines():
        m = re.match(r"^([0-9a-f]+) <(.*)>:$", line)
        if m:
            name = m.group(2)
            table[name] = []
            continue
        if name is None or not line.strip() or "file format" in line or line.startswith("Disassembly of section"):
            continue
        ins = re.sub(r"//.*$", "", line).strip()
        ins = re.sub(r"<[^>]*\+0x([0-9a-f]+)>", lambda k: "<+" + k.group(1) + ">", ins)     # branch targets: offsets in the kernel
        ins = re.sub(r"^\s*[0-9a-f]+:\s*", "", ins)
        if ins == "...":                                       # objdump's elision of padding behind the last kernel
            continue
        # pc-relative address arithmetic (s_getpc_b64, then s_add_u32 / s_addc_u32 with a literal): depends on where the
        # linker put the kernel, not on its code
        pcrel = 3 if ins.startswith("s_getpc_b64") else pcrel - 1
        if 0 < pcrel < 3 and ins.startswith(("s_add_u32", "s_addc_u32")):
            ins = re.sub(r"0x[0-9a-f]+$", "<pcrel>", ins)
        table[name].append(ins)
    return table


def main():
    old, new = sys.argv[1], sys.argv[2]
    renames = [a.split("=", 1) for a in sys.argv[3:] if "=" in a]
    rest = [a for a in sys.argv[3:] if "=" not in a]
    rx = re.compile(rest[0] if rest else ".")
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "a")); os.makedirs(os.path.join(tmp, "b"))
        ka, kb = kernels(code_objects(old, os.path.join(tmp, "a"))), kernels(code_objects(new, os.path.join(tmp, "b")))
    for old_type, new_type in renames:
        ka = {re.sub(r"\b%s\b" % re.escape(old_type), new_type, n): v for n, v in ka.items()}
    common = sorted(n for n in ka if n in kb and rx.search(n))
    differ = [n for n in common if ka[n] != kb[n]]
    for n in differ:
        print("DIFFERS ", n)
    for n in sorted(set(kb) - set(ka)):
        if rx.search(n):
            print("NEW     ", n)
    for n in sorted(set(ka) - set(kb)):
        if rx.search(n):
            print("GONE    ", n)
    print(f"{len(common)} common kernels matching, {len(common) - len(differ)} identical, {len(differ)} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
