#!/usr/bin/env python3
"""Per-kernel instruction streams of the gfx950 code objects inside a built librpf_engine.so, and their comparison
between two builds:

    tools/kernel_streams.py LIB                 one line per kernel: sha256 of its instruction stream, length, name
    tools/kernel_streams.py PARENT_LIB LIB      which kernels of PARENT_LIB are instruction for instruction in LIB

The library's .hip_fatbin section holds one offload bundle per translation unit; each is unbundled for gfx950 and
disassembled (llvm-objdump -d, addresses and encodings dropped, so only mnemonics and operands count).  Kernels are
matched by demangled name; the trailing `, false` a defaulted `bool STATS` adds to the two K1 kernel templates'
argument lists is dropped before matching, so that a build with that parameter can be compared with one before it;
so is the `, 0` of the defaulted `int LDW` behind it (a kernel with loader waves keeps its `, 1` or `, 2`: it is a new
kernel, and the one it replaced is reported as different or missing); and so is the `, false, 0, false` that follows
the sixth template argument (DMA, counting N and P of the Geom apart) of every K1 accumulate kernel (`fft_accum_*kernel<`)
in a build that still has the three retired experiments' parameters ("Retired experiments"), so that such
a build can be compared with one without them."""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def streams(lib):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fatbin")
        subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
        for k, st in enumerate(starts):
            end = starts[k + 1] if k + 1 < len(starts) else len(blob)
            bundle, co = os.path.join(tmp, "b%d" % k), os.path.join(tmp, "c%d.co" % k)
            open(bundle, "wb").write(blob[st:end])
            r = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=" + TARGET,
                                "--input=" + bundle, "--output=" + co, "--unbundle"], capture_output=True, text=True)
            if r.returncode != 0:
                continue                        # a bundle without a gfx950 entry (host-only unit)
            text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co],
                                  capture_output=True, text=True, check=True).stdout
            cur = None
            for line in text.splitlines():
                line = line.strip()
                m = re.match(r"^(?:[0-9a-f]+ )?<([^>]+)>:$", line)
                if m:
                    cur = m.group(1)
                    out[cur] = []
                elif cur and line and "file format" not in line and not line.startswith("Disassembly of"):
                    out[cur].append(re.sub(r"\s*//.*$", "", line))
    names = list(out)
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    res = {}
    for mangled, name in zip(names, plain):
        # the three retired experiments' parameters behind <Geom<N, P>, WG, OCC, WINDOW, DMA
        name = re.sub(r"(fft_accum_\w*kernel<rpf::Geom<\d+, \d+>, \d+, \d+, (?:false|true), (?:false|true))"
                      r", false, 0, false", r"\1", name)
        if "fft_accum_kernel<" in name:
            name = re.sub(r", (false|true), 0>\(", r", \1>(", name)      # the defaulted `int LDW` behind STATS
        if "fft_accum_kernel<" in name or "fft_accum_strided_kernel<" in name:
            name = re.sub(r", false>\(", ">(", name)
        res[name] = (hashlib.sha256("\n".join(out[mangled]).encode()).hexdigest(), len(out[mangled]))
    return res


def main():
    if len(sys.argv) == 2:
        for name, (h, n) in sorted(streams(sys.argv[1]).items()):
            print(h[:16], n, name)
        return 0
    a, b = streams(sys.argv[1]), streams(sys.argv[2])
    k1 = [n for n in a if "fft_accum" in n]
    other = [n for n in a if n not in k1]
    rep = {"parent_kernels": len(a), "kernels": len(b),
           "k1_parent": len(k1), "k1_identical": sum(1 for n in k1 if b.get(n) == a[n]),
           "k1_instructions": sum(a[n][1] for n in k1),
           "other_parent": len(other), "other_identical": sum(1 for n in other if b.get(n) == a[n]),
           "new_kernels": sum(1 for n in b if n not in a),
           "different_or_missing": sorted(n for n in a if b.get(n) != a[n])}
    print(json.dumps(rep, indent=1))
    return 0 if not rep["different_or_missing"] else 1


if __name__ == "__main__":
    sys.exit(main())
