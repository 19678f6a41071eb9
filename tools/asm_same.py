#!/usr/bin/env python3
"""Compare two device assemblies kernel by kernel: the same symbols, and for each the same instruction text (label to
s_endpgm) and the same resource block (registers, LDS, scratch, occupancy).  The order of the symbols may differ.
usage: hipcc <the Makefile's flags> --cuda-device-only -S OLD.hip -o old.s; the same for NEW; python tools/asm_same.py old.s new.s"""
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from test_kernel_resources import kernels  # noqa: E402

RES = re.compile(r"^; (?:NumSgprs|NumVgprs|NumAgprs|TotalNumVgprs|ScratchSize|Occupancy|LDSByteSize|codeLenInByte|"
                 r"SGPRBlocks|VGPRBlocks|NumSGPRsForWavesPerEU|NumVGPRsForWavesPerEU).*$", re.M)
a, b = (kernels(open(p).read()) for p in sys.argv[1:3])
bad = sorted(set(a) ^ set(b))
for k in sorted(set(a) & set(b)):
    if a[k][0] != b[k][0] or RES.findall(a[k][1]) != RES.findall(b[k][1]) or not RES.findall(a[k][1]):
        bad.append(k)
    else:
        print("same  %s  %d lines  %s" % (k, a[k][0].count("\n") + 1, " ".join(
            m.lstrip("; ") for m in RES.findall(a[k][1]) if re.match(r"; (NumVgprs|NumSgprs|ScratchSize|Occupancy|LDSByteSize)", m))))
print("%d kernels in %s, %d in %s, %d differ or are missing%s" % (len(a), sys.argv[1], len(b), sys.argv[2], len(bad),
                                                                   (": " + " ".join(bad)) if bad else ""))
sys.exit(1 if bad or not a else 0)
