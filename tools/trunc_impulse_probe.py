#!/usr/bin/env python3
"""Developer probe: impulse responses of the serial PADDED plans (3/2-rule truncating store forward, zero-padding load backward;
tests/cases.py trunc_impulse_errors: unit impulses and single stored bins against their exact answers, every line of the
batch) in units of eps * log2 n of the exact answer's peak, per path (the fused adapters of the register kernels / the
stand-alone trunc_kernel), mapping, padded length -> kept length and dtype -- and beside each the UNPADDED plan of the same
length, mapping and dtype on the same impulse positions and bins: what IMPULSE_FACTOR of tests/test_gpu_trunc_guard.py is
held against (profiles/trunc_impulse_probe.txt)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from tests import cases

worst, plain = {}, {}
for dt in 'DFdf':
    for mapping in cases.TRUNC_MAPPINGS:
        for n, kept, family in cases.TRUNC_CASES:
            text = []
            ef, eb = cases.trunc_impulse_errors(n, kept, dt, mapping, describe=text)
            path = cases.trunc_path(text, n, mapping)
            if (n, dt, mapping) not in plain:
                plain[n, dt, mapping] = cases.trunc_impulse_errors(n, n, dt, mapping)
            uf, ub = plain[n, dt, mapping]
            u = cases.EPS[dt] * np.log2(n)
            print('%s %-6s %5d -> %-5d %-11s fwd %.2e (%.2f)  bwd %.2e (%.2f)   unpadded fwd %.2f  bwd %.2f%s'
                  % (dt, mapping, n, kept, path, ef, ef / u, eb, eb / u, uf / u, ub / u,
                     '' if path in cases.trunc_expected_path(n, family, dt, mapping) else '  [expected %s]' % family), flush=True)
            key = (path, 'fp64' if dt in 'Dd' else 'fp32')
            if max(ef, eb) / u > worst.get(key, (-1,))[0]:
                worst[key] = (max(ef, eb) / u, max(uf, ub) / u, dt, mapping, n, kept)
print('worst per path (eps log2 n of the peak), with the unpadded plan of the same length, mapping and dtype beside it:')
for key in sorted(worst):
    print('  %-11s %s  %.2f   unpadded %.2f   (%s %s %d -> %d)' % (key + worst[key]))
for prec in ('fp64', 'fp32'):
    print('worst over the family, %s: padded %.2f, unpadded %.2f' % (prec, max(v[0] for k, v in worst.items() if k[1] == prec),
                                                                      max(max(p) / (cases.EPS[k[1]] * np.log2(k[0])) for k, p in plain.items()
                                                                          if (k[1] in 'Dd') == (prec == 'fp64'))))
