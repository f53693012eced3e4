#!/usr/bin/env python3
"""Compare the device code of two builds, kernel by kernel.

Each directory holds one gfx950 ELF per source file of the Makefile's SRCS, compiled with the Makefile's flags plus
`--cuda-device-only --no-gpu-bundle-output -c`.  Over the union of the files of a directory, a kernel is a FUNC symbol
NAME with an OBJECT symbol NAME.kd (its 64-byte descriptor).  Reports kernels present on one side only and kernels whose
code bytes or descriptor bytes differ; only names and bytes are compared (which file a kernel sits in is not).  Bytes 16-23
of a descriptor (kernel_code_entry_byte_offset: the distance from the descriptor to the code inside its file) say where the
linker put the two, not what the kernel is, and move whenever a neighbour in the file does: they are left out.

A change that removes a template parameter changes the mangled names: --rename-a 'REGEX=REPLACEMENT' (repeatable; re.sub on every kernel
name of DIR_A, in the order given) states the pairing rule on the command line.

usage: compare_device_code.py DIR_A DIR_B [--readelf /opt/rocm/llvm/bin/llvm-readelf] [--rename-a REGEX=REPL ...] [--all]
"""
import argparse
import pathlib
import re
import subprocess
import sys


def kernels(directory, readelf):
    out = {}
    for elf in sorted(pathlib.Path(directory).glob("*.elf")):
        data = elf.read_bytes()
        text = subprocess.run([readelf, "-SW", "-sW", str(elf)], check=True, capture_output=True, text=True).stdout
        sections, symbols = {}, {}
        for line in text.splitlines():
            f = line.replace("[", " ").replace("]", " ").split()
            if len(f) >= 6 and f[0].isdigit() and f[1].startswith("."):          # section: ndx name type addr off size
                sections[int(f[0])] = (int(f[3], 16), int(f[4], 16))
            elif len(f) == 8 and f[0].endswith(":") and f[3] in ("FUNC", "OBJECT") and f[6].isdigit():
                symbols[f[7]] = (int(f[1], 16), int(f[2]), f[3], int(f[6]))        # value size type section

        def blob(name):
            value, size, _, ndx = symbols[name]
            addr, off = sections[ndx]
            return data[off + value - addr: off + value - addr + size]

        for name, (_, _, typ, _) in symbols.items():
            if typ == "FUNC" and name + ".kd" in symbols:
                assert name not in out, "kernel defined twice: " + name
                kd = blob(name + ".kd")
                assert len(kd) == 64, name
                out[name] = (blob(name), kd[:16] + kd[24:])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir_a")
    ap.add_argument("dir_b")
    ap.add_argument("--readelf", default="/opt/rocm/llvm/bin/llvm-readelf")
    ap.add_argument("--rename-a", action="append", default=[], metavar="REGEX=REPL")
    ap.add_argument("--all", action="store_true", help="print every name of a list, not the first 20")
    a = ap.parse_args()
    ka, kb = kernels(a.dir_a, a.readelf), kernels(a.dir_b, a.readelf)
    renamed = {}
    for name, blobs in ka.items():
        new = name
        for rule in a.rename_a:
            pat, _, repl = rule.partition("=")
            new = re.sub(pat, repl, new)
        assert new not in renamed, "two kernels of A renamed to " + new
        renamed[new] = blobs
    if a.rename_a:
        print(f"renamed in A: {sum(1 for n in renamed if n not in ka)}")
    ka = renamed
    only_a, only_b = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
    code = [n for n in sorted(set(ka) & set(kb)) if ka[n][0] != kb[n][0]]
    desc = [n for n in sorted(set(ka) & set(kb)) if ka[n][1] != kb[n][1]]
    print(f"kernels: {len(ka)} in {a.dir_a}, {len(kb)} in {a.dir_b}")
    print(f"code bytes compared: {sum(len(v[0]) for v in ka.values())} / {sum(len(v[0]) for v in kb.values())}")
    for title, names in (("only in A", only_a), ("only in B", only_b), ("code differs", code), ("descriptor differs", desc)):
        print(f"{title}: {len(names)}")
        for n in names if a.all else names[:20]:
            print("   ", n)
    return 1 if (only_a or only_b or code or desc) else 0


if __name__ == "__main__":
    sys.exit(main())
