#!/usr/bin/env python3
"""Developer probe: impulse responses of the serial REAL-TO-REAL plans (DCT / DST I-IV; tests/cases.py r2r_impulse_errors:
unit impulses against their exact answers, every line of the batch) in units of 2 eps * log2 N -- 2 being the exact answer's
peak --, per kind, logical length, mapping and precision, with the path gfft_plan_describe names (the MODE_R2R adapters of
the register kernels / the embed ... extract fallback / the same through Bluestein) -- and the worst ratio per path: what
R2R_IMPULSE_FACTOR of tests/test_gpu_r2r_guard.py is held against (profiles/r2r_impulse_probe.txt)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from tests import cases

worst = {}
for dt in 'df':
    for mapping in cases.R2R_MAPPINGS:
        for want, lengths in cases.R2R_LENGTHS.items():
            for N in lengths:
                for kind in sorted(cases.R2R_NAMES):
                    text = []
                    err = cases.r2r_impulse_errors(kind, N, dt, mapping, describe=text)
                    path = cases.r2r_path(text, N, mapping)
                    u = 2 * cases.EPS[dt] * np.log2(N)
                    print('%s %-6s N=%-5d %-9s %s  %.2e (%.2f x 2 eps log2 N)%s' % (dt, mapping, N, path, cases.R2R_NAMES[kind], err, err / u,
                                                                                  '' if path == want else '  [expected %s]' % want), flush=True)
                    key = (path, mapping, dt)
                    if err / u > worst.get(key, (-1,))[0]:
                        worst[key] = (err / u, cases.R2R_NAMES[kind], N)
print('worst per path (2 eps log2 N):')
for key in sorted(worst):
    print('  %-9s %-6s %s  %.2f (%s, N = %d)' % (key + worst[key]))
print('worst over the family: %.2f (fp64), %.2f (fp32)' % tuple(max(v[0] for k, v in worst.items() if k[2] == dt) for dt in 'df'))
