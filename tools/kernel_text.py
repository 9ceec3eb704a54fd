#!/usr/bin/env python3
"""Per-kernel code identity of one .hip source as hipcc compiles it for gfx950 (no GPU needed): one line per kernel with
its demangled name, its size, a hash of the function's .text bytes and a hash of its 64-byte kernel descriptor (the
entry-offset field, bytes 16-23, zeroed: it moves with link order).  Two trees whose listings agree run the same device
code; a byte comparison only, no instruction is looked at.
    python tools/kernel_text.py pair_reproject [extra hipcc flags]"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/llvm/bin/"
src = sys.argv[1]
with tempfile.TemporaryDirectory() as tmp:
    bundle, elf = os.path.join(tmp, "dev.o"), os.path.join(tmp, "dev.elf")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", *sys.argv[2:],
                    "--cuda-device-only", "-c", src + ".hip", "-o", bundle],
                   cwd=os.path.join(ROOT, "multi-spatialmllm_amd", "csrc"), check=True)
    subprocess.run([LLVM + "clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--input=" + bundle, "--output=" + elf], check=True)
    blob = open(elf, "rb").read()
    if blob[:4] != b"\x7fELF":      # hipcc -c --cuda-device-only may write the code object unbundled
        blob = open(bundle, "rb").read()
        elf = bundle
    sections = {}                   # index -> (address, file offset)
    for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S*\s+\S+\s+([0-9a-f]{16})\s+([0-9a-f]+)\s", subprocess.run(
            [LLVM + "llvm-readelf", "-S", "-W", elf], capture_output=True, text=True, check=True).stdout, re.M):
        sections[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))
    funcs, descs = {}, {}
    for line in subprocess.run([LLVM + "llvm-readelf", "-s", "-W", elf], capture_output=True, text=True, check=True).stdout.splitlines():
        f = line.split()
        if len(f) != 8 or f[3] not in ("FUNC", "OBJECT") or not f[6].isdigit():
            continue
        addr, size, (sec_addr, sec_off) = int(f[1], 16), int(f[2]), sections[int(f[6])]
        data = blob[addr - sec_addr + sec_off:addr - sec_addr + sec_off + size]
        if f[3] == "FUNC":
            funcs[f[7]] = data
        elif f[7].endswith(".kd") and size == 64:
            descs[f[7][:-3]] = data[:16] + bytes(8) + data[24:]

names = sorted(funcs)
pretty = subprocess.run(["c++filt", *names], capture_output=True, text=True).stdout.splitlines()
for name, p in sorted(zip(names, pretty), key=lambda t: t[1]):
    p = re.sub(r"\(.*", "", re.sub(r"^(void )?mspa::", "", p))       # the parameter list says nothing the name does not
    kd = hashlib.sha256(descs[name]).hexdigest()[:16] if name in descs else "-" * 16
    print("%-100s size %6d text %s kd %s" % (p[:100], len(funcs[name]), hashlib.sha256(funcs[name]).hexdigest()[:16], kd))
print("%d functions, %d kernel descriptors" % (len(funcs), len(descs)))
