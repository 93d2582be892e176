#!/usr/bin/env python3
"""Developer probe (round 8): does the order IN TIME in which the stand-alone strided fp64 pass of the 1024^3 complex128
schedule requests its tiles and rows (option tile_order = PassDesc::order, gfft_internal.h) move its time?  One plan, the
orders alternating on the SAME arrays (the option is read at launch time), over several freshly allocated array sets --
placement is the variable under study -- in both directions (forward reads the physical array, backward the spectral one;
both write the tile-major workspace).  With GFFT_AB_LIB naming a library whose fft_pow2_f64 was built with -DGFFT_VARIANTS,
the ACCESS PATTERN ALONE of the same kernel (variant_cols 11: loads and stores, no butterflies, no exchange) is measured too.
usage: [GFFT_AB_LIB=libgfft_var.so] tile_order_probe.py [array sets, default 6] [launches per sample, default 4] [orders, comma separated]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpi4py_fft_amd import _lib
if os.environ.get('GFFT_AB_LIB'):
    _lib.LIBPATH = os.path.join(os.path.dirname(_lib.LIBPATH), os.environ['GFFT_AB_LIB'])
import torch
from mpi4py_fft_amd import PFFT, newDistArray, comm

n = 1024
nsets = int(sys.argv[1]) if len(sys.argv) > 1 else 6
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 4


def label(o):
    """PassDesc::order in words (gfft_internal.h)."""
    parts = []
    if o & 4095: parts.append('a XCD start x*%d' % (o & 4095))
    if (o >> 12) & 3: parts.append('b %d slot rotations' % (2 * ((o >> 12) & 3)))
    if (o >> 14) & 3: parts.append('b thread rows +%d*h' % (5 if ((o >> 14) & 3) == 1 else 4))
    if (o >> 16) & 3: parts.append('c %d planes %d apart' % (1 << ((o >> 16) & 3), ((o >> 19) & 127) or 37))
    if (o >> 18) & 1: parts.append('h=XCD+k')
    return ', '.join(parts) or 'plain'


Q2, Q4, ROT5, ROT4, IL2, IL4, HK = 1 << 12, 2 << 12, 1 << 14, 2 << 14, 1 << 16, 2 << 16, 1 << 18
# a: 64*3+5, 64*5+3, 64*7+1 tiles;  d: combinations
default = [0, 197, 323, 449, Q2, Q4, Q4 | HK, ROT5 | HK, ROT4, IL2, IL4, 197 | Q4, 323 | IL2 | Q4]
orders = [(label(o), o) for o in ([0] + [int(x, 0) for x in sys.argv[3].split(',')] if len(sys.argv) > 3 else default)]
variants = [0, 11] if os.environ.get('GFFT_AB_LIB') else [0]
ffts = {}
for v in variants:
    _lib.set_option('variant_cols', v)
    ffts[v] = PFFT(comm.COMM_SELF, (n,) * 3, dtype='D')
_lib.set_option('variant_cols', 0)
print(torch.cuda.get_device_name(0), '| 1024^3 complex128, stand-alone axis-1 pass, ms per launch (mean of %d)' % reps, flush=True)


def pass_ms(f, direction, u, w):
    run = (lambda: f.forward(u, w)) if direction == 0 else (lambda: f.backward(w, u))
    run()
    _lib.set_option('profile', 1)
    for _ in range(reps):
        run()
    torch.cuda.synchronize()
    _lib.set_option('profile', 0)
    out = {}
    for name, nb, ms, k in f._fused_plans[direction].profile():
        out[name.split(' n=')[0].strip()] = ms / max(k, 1)
    return out


res = {}          # (variant, direction, label) -> [per set: pass ms]
pair = {}
keep = []
for s in range(nsets):
    u, w = newDistArray(ffts[0], False), newDistArray(ffts[0], True)
    torch.view_as_real(u.tensor).normal_()
    for v, f in ffts.items():
        for direction in (0, 1):
            for name, o in orders:
                _lib.set_option('tile_order', o)
                t = pass_ms(f, direction, u, w)
                _lib.set_option('tile_order', -1)
                cols = [x for k, x in t.items() if 'pow2-cols' in k]
                res.setdefault((v, direction, name), []).append(cols[0])
                pair.setdefault((v, direction, name), []).append(sum(x for k, x in t.items() if 'fused' in k))
    print('array set %d done (u at %#x, w at %#x)' % (s, u.tensor.data_ptr(), w.tensor.data_ptr()), flush=True)
    # the next set must not land on the same pages: the old arrays go back to the driver, an odd-sized spacer stays
    del u, w
    torch.cuda.empty_cache()
    keep.append(torch.empty((1 << 30) + (2 * s + 3) * (2 << 20) + 4096 * (s + 1), dtype=torch.uint8, device='cuda'))
for v in ffts:
    for direction in (0, 1):
        print('--- variant_cols %d (%s), %s' % (v, 'the kernel' if v == 0 else 'its access pattern alone', 'forward' if direction == 0 else 'backward'))
        base = res[(v, direction, 'plain')]
        print('%-44s %s   spread of the plain order over the sets: %.3f ms' % ('', ' '.join('set%-4d' % i for i in range(nsets)), max(base) - min(base)))
        for name, o in orders:
            ts = res[(v, direction, name)]
            d = [a - b for a, b in zip(ts, base)]
            print('%-44s %s   mean %.3f   vs plain: mean %+.3f  best %+.3f  worst %+.3f   (pair %.3f)' % (
                name + ' [%d]' % o, ' '.join('%7.3f' % t for t in ts), sum(ts) / len(ts), sum(d) / len(d), min(d), max(d),
                sum(pair[(v, direction, name)]) / nsets))
