#!/usr/bin/env python3
"""Developer probe: impulse responses of the serial REAL plans (tests/cases.py real_impulse_errors: r2c of unit impulses,
c2r of single bins, against their exact answers) in units of eps * log2 n, per length, precision and mapping, with the
kernel family gfft_plan_describe names -- and the worst ratio per family: what REAL_IMPULSE_FACTOR of
tests/test_gpu_rounding_guard.py was set from (profiles/real_impulse_probe.txt)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from tests import cases

worst = {}
for dt in 'DF':
    for strided in (False, True):
        for n, _ in cases.REAL_ROWS:
            text = []
            ef, eb = cases.real_impulse_errors(n, dt, strided, describe=text)
            path = cases.real_path(text)
            u = cases.EPS[dt] * np.log2(n)
            m = 'strided' if strided else 'rows'
            print('%s %-7s n=%-6d %-9s fwd %.2e (%.2f eps log2 n)  bwd %.2e (%.2f)' % (dt, m, n, path, ef, ef / u, eb, eb / u), flush=True)
            for d, e in (('fwd', ef), ('bwd', eb)):
                key = (path, m, dt, d)
                if e / u > worst.get(key, (-1, 0))[0]:
                    worst[key] = (e / u, n)
print('worst per kernel family (eps log2 n):')
for key in sorted(worst):
    print('  %-9s %-7s %s %s  %.2f (n = %d)' % (key + worst[key]))
print('worst over the family: %.2f' % max(v[0] for v in worst.values()))
