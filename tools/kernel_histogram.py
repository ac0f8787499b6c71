#!/usr/bin/env python3
"""Instructions per mnemonic of every kernel in one csrc file (device assembly; no GPU needed):
    tools/kernel_histogram.py conv_mfma.hip > after.txt     # diff against the same on the parent commit
Labels, directives and comments are ignored; register numbers and instruction order do not show.  Next to
tools/kernel_resources.sh this is the check that a source-level refactor left the generated kernels alone."""
import collections
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from face_vijnana_yolov3_amd.build import CSRC, FLAGS, HIPCC

asm = subprocess.run([HIPCC] + FLAGS + ['--cuda-device-only', '-S', os.path.join(CSRC, sys.argv[1]), '-o', '-'],
                     check=True, capture_output=True, text=True).stdout
kernels = re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', asm, re.M)
names = subprocess.run(['c++filt'] + kernels, check=True, capture_output=True, text=True).stdout.split('\n')
for sym, name in sorted(zip(kernels, names), key=lambda p: p[1]):
    body = asm.split('\n' + sym + ':', 1)[1].split('.Lfunc_end', 1)[0]
    hist = collections.Counter()
    for line in body.split('\n'):
        line = line.split(';', 1)[0].strip()
        if line and not line.startswith('.') and not line.endswith(':'):
            hist[line.split()[0]] += 1
    print('%s  (%d instructions)' % (name.replace('(anonymous namespace)::', ''), sum(hist.values())))
    for m in sorted(hist):
        print('    %-28s %d' % (m, hist[m]))
