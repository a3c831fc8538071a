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
a build can be compared with one without them; and so is the `, 2, 0` of the defaulted `int NBUF, int NT` at the end of
the fused four-step kernel's (`fourstep_fused_kernel<`) argument list in a build that still has those two retired
experiments' parameters (Four-step, "Retired experiments": a kernel with another value, `, 1, 0` say, keeps
it and is reported as different or missing).

A kernel reaches its constant tables through a pc-relative address: `s_getpc_b64 s[LO:HI]`, then `s_add_u32 sLO, sLO,
<literal>` / `s_addc_u32 sHI, sHI, <literal>`.  The literal is the distance from the instruction to the table and moves
whenever the code object's layout does (a shorter mangled name is enough), with no instruction of the kernel changed.
A second digest of every stream is therefore taken with the literals of exactly that pair masked -- the same
instructions anywhere else, or on other registers, are left as they are -- and the two-library report counts and NAMES
the kernels that are identical only under it (`identical_but_for_pc_relative_literal`), so that the mask cannot
silently swallow a real difference."""
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


def drop_fused_defaults(name):
    """The demangled name without the `, 2, 0` of `fourstep_fused_kernel`'s retired `int NBUF = 2, int NT = 0`."""
    if "fourstep_fused_kernel<" not in name:
        return name
    return re.sub(r", 2, 0>\(", ">(", name)


PCREL = "<pc-relative>"


def mask_pc_relative(lines):
    """The instruction lines with the literals of `s_add_u32 sLO, sLO, <literal>` / `s_addc_u32 sHI, sHI, <literal>`
    masked where the pair directly follows `s_getpc_b64 s[LO:HI]`; every other line as it is."""
    out = list(lines)
    for i, line in enumerate(lines):
        m = re.match(r"^s_getpc_b64 s\[(\d+):(\d+)\]$", line)
        if not m:
            continue
        pair = ["%s s%s, s%s, " % (op, reg, reg) for op, reg in (("s_add_u32", m.group(1)), ("s_addc_u32", m.group(2)))]
        if all(re.match(re.escape(head) + r"\S+$", nxt) for head, nxt in zip(pair, lines[i + 1:i + 3] + ["", ""])):
            out[i + 1:i + 3] = [head + PCREL for head in pair]
    return out


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def streams(lib):
    """{demangled name: (digest of the stream, its length, digest with the pc-relative literals masked)}"""
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
        name = drop_fused_defaults(name)
        res[name] = (digest(out[mangled]), len(out[mangled]), digest(mask_pc_relative(out[mangled])))
    return res


def main():
    if len(sys.argv) == 2:
        for name, (h, n, _) in sorted(streams(sys.argv[1]).items()):
            print(h[:16], n, name)
        return 0
    a, b = streams(sys.argv[1]), streams(sys.argv[2])
    k1 = [n for n in a if "fft_accum" in n]
    other = [n for n in a if n not in k1]
    pcrel = sorted(n for n in a if n in b and b[n] != a[n] and b[n][2] == a[n][2])
    rep = {"parent_kernels": len(a), "kernels": len(b),
           "k1_parent": len(k1), "k1_identical": sum(1 for n in k1 if b.get(n) == a[n]),
           "k1_instructions": sum(a[n][1] for n in k1),
           "other_parent": len(other), "other_identical": sum(1 for n in other if b.get(n) == a[n]),
           "identical_but_for_pc_relative_literal": len(pcrel),
           "identical_but_for_pc_relative_literal_names": pcrel,
           "new_kernels": sum(1 for n in b if n not in a),
           "different_or_missing": sorted(n for n in a if b.get(n) != a[n] and n not in pcrel)}
    print(json.dumps(rep, indent=1))
    return 0 if not rep["different_or_missing"] else 1


if __name__ == "__main__":
    sys.exit(main())
