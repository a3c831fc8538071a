#!/usr/bin/env python3
"""Summarise hipcc -Rpass-analysis=kernel-resource-usage output (stdin)."""
import re, sys
cur = None
d = {}
for l in sys.stdin:
    if 'error' in l or 'warning' in l:
        print(l.rstrip())
    m = re.search(r'Function Name: (\S+)', l)
    if m:
        cur = m.group(1); d = {}; continue
    m = re.search(r':\s+([A-Za-z][A-Za-z ]*?)(?: \[[^\]]*\])?: (\d+) \[-Rpass', l)
    if m and cur:
        d[m.group(1).strip()] = m.group(2)
        if 'LDS Size' in m.group(1):
            g = re.search(r'GeomILi(\d+)ELi(\d+)EEELi(\d+)ELi(\d+)ELb(\d)ELb(\d)', cur)
            tag = 'N=%s P=%s WG=%s OCC=%s win=%s dma=%s' % g.groups() if g else cur[:48]
            f = re.search(r'pfb_fold_(sliding|reread)_kernelILi(\d+)E(?:Li(\d+)E)?Lb(\d)E', cur)
            if f:
                tag = 'pfb_fold %s fmt=%s taps=%s aligned=%s' % (f.group(1), f.group(2), f.group(3) or 'any', f.group(4))
            f = re.search(r'cross_combine_kernelILi(\d+)ELb(\d)ELb(\d)E', cur)
            if f:
                tag = 'cross_combine fmt=%s aligned_a=%s aligned_b=%s' % f.groups()
            elif 'cross_finish_kernel' in cur:
                tag = 'cross_finish'
            f = re.search(r'fft_stft(_strided)?_kernelINS_4GeomILi(\d+)ELi(\d+)EEELi(\d+)ELi(\d+)ELb(\d)ELb(\d)ELi(\d+)ELb(\d)ELi(\d+)E', cur)
            if f:
                tag = 'stft%s N=%s P=%s WG=%s OCC=%s win=%s dma=%s rawd=%s twlds=%s fmt=%s' % ((f.group(1) or '',) + f.groups()[1:])
            f = re.search(r'correlate_xengine_kernelILi(\d+)E', cur)
            if f:
                tag = 'correlate_xengine M=%s' % f.group(1)
            elif 'correlate_reduce_kernel' in cur or 'correlate_finish_kernel' in cur:
                tag = re.search(r'(correlate_\w+?)_kernel', cur).group(1)
            if 'dedisperse_kernel' in cur:
                tag = 'dedisperse LDS=%s' % m.group(2)
            f = re.search(r'\d\dfold_(reduce_)?kernel(?:ILb(\d)E)?', cur)
            if f:
                tag = 'fold_reduce' if f.group(1) else ('fold series' if f.group(2) == '1' else 'fold hits') + ' (LDS is dynamic)'
            print(tag, {k: d.get(k) for k in ('VGPRs', 'AGPRs', 'ScratchSize', 'Occupancy', 'VGPRs Spill')})
