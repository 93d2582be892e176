#!/usr/bin/env python3
"""What the planner decides, as text: for a fixed list of requests -- the shapes of the fused pairs and their neighbours, and a few
small requests through every other plan creator (guru, padded, r2r, one line per family of lengths) --, once under
the defaults and once under each planning option that switches a pair -- gfft_plan_describe, every pass's name and bytes
(gfft_plan_pass_info) and gfft_plan_cost; under an option, only the requests that come out other than under the defaults are
printed.  Plans are created and destroyed, nothing is allocated or executed: seconds on a GPU.
Two builds whose outputs are identical plan identically: what a refactor of plan.cpp / api.cpp / the pair tables has to show.
--brief: one line per request instead -- its passes under the defaults, a digest (sha256, 12 digits) of the full text above, and
the digest under every option that changes it: the form that is kept under profiles/.
usage: plan_fingerprint.py [--brief] > out.txt   (GFFT_AB_LIB=<file next to libgfft.so>: under that build of the library)"""
import ctypes, hashlib, os, re, sys
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
from mpi4py_fft_amd import _lib
if os.environ.get('GFFT_AB_LIB'):
    _lib.LIBPATH = os.path.join(os.path.dirname(_lib.LIBPATH), os.environ['GFFT_AB_LIB'])
eng = _lib.engine()
FWD, BWD, R2C, C2R = _lib.C2C_FORWARD, _lib.C2C_BACKWARD, _lib.R2C, _lib.C2R
DEFAULTS = {'fuse2': 1, 'fuse2_kinds': 2046, 'fuse2_f32': 1, 'wtile': 1, 'fuse2_n512': 2, 'fuse2_mixed': 1, 'fuse2_mixv': 1,
            'fuse2_f32_n512': 1, 'c2r_2048': 1, 'fuse2_ring': 0, 'fuse2_lag': 0}
OPTIONS = [{}, {'fuse2': 0}, {'fuse2_kinds': 1}, {'fuse2_kinds': 15}, {'fuse2_f32': 0}, {'fuse2_f32': 2}, {'wtile': 0}, {'wtile': 2},
           {'fuse2_n512': 0}, {'fuse2_n512': 1}, {'fuse2_mixed': 0}, {'fuse2_mixv': 0}, {'fuse2_f32_n512': 0}, {'c2r_2048': 0},
           {'fuse2_ring': 8, 'fuse2_lag': 4}]


def fingerprint(make):
    try:
        h = make()
    except _lib.GfftError as e:
        return '   error: %s\n' % e
    if h is None:
        return '   unsupported\n'
    text = eng.plan_describe(h)
    for i in range(int(re.search(r'(\d+) passes', text).group(1))):
        buf, b = ctypes.create_string_buffer(64), ctypes.c_double()
        _lib.check(_lib.lib().gfft_plan_pass_info(h, i, buf, 64, ctypes.byref(b)))
        text += '   pass %d: %s, %r bytes\n' % (i, buf.value.decode(), b.value)
    text += '   cost: %r flops, %r bytes, %d launches\n' % eng.plan_cost(h)
    eng.plan_destroy(h)
    return text


def requests():
    half = lambda s: s[:-1] + (s[-1] // 2 + 1,)
    for prec in (8, 4):
        for s in ((1024,) * 3, (512,) * 3, (512, 1024, 1024), (1024, 1024, 512), (1024, 16, 1024), (1024, 40, 1024), (960,) * 3,
                  (896,) * 3, (768,) * 3):
            for kind in (FWD, BWD):
                yield 'c2c %+d f%d %s axes (0,1,2)' % (kind, 8 * prec, s), lambda s=s, kind=kind: eng.plan_create(s, s, (0, 1, 2), kind, prec)
        # (the last shape: rows of 769 entries, not whole lines wide -- the flat_out schedule on a 3 x 2^k length)
        for s in ((1024,) * 3, (1024, 1024, 2048), (40, 1024, 1024), (1024, 40, 1024), (256, 1024, 1536)):
            yield 'r2c f%d %s' % (8 * prec, s), lambda s=s: eng.plan_create(s, half(s), (0, 1, 2), R2C, prec)
            yield 'c2r f%d %s' % (8 * prec, s), lambda s=s: eng.plan_create(half(s), s, (0, 1, 2), C2R, prec)
        for s, axes in (((32, 1 << 20), (1,)), ((64, 1 << 20), (1,)), ((256, 1024, 1024), (1, 2)), ((256, 512, 512), (1, 2))):
            for kind in (FWD, BWD):
                yield 'c2c %+d f%d %s axes %s' % (kind, 8 * prec, s, axes), lambda s=s, axes=axes, kind=kind: eng.plan_create(s, s, axes, kind, prec)
        # the two local stages of a slab-decomposed transform: 256 planes of n1 x n2 points, the strided axis in blocks on one side
        planes = 256
        for n1, n2 in ((1024, 1024), (512, 512), (512, 1024), (1024, 512)):
            for cf in (False, True):
                for kind in (FWD, BWD):
                    for inb, outb in ((1, 1), (4, 1), (1, 4)):
                        E = n1 // max(inb, outb) * n2 + 16           # one plane of one block, planes 16 entries apart
                        pin = (n1 * n2, 0) if inb == 1 else (E, planes * E)
                        pout = (n1 * n2, 0) if outb == 1 else (E, planes * E)
                        yield ('guru2 %+d f%d %dx%d cols_first=%d blocks %d -> %d' % (kind, 8 * prec, n1, n2, cf, inb, outb),
                               lambda n1=n1, n2=n2, cf=cf, kind=kind, inb=inb, outb=outb, pin=pin, pout=pout:
                               eng.plan_create_guru2(prec, kind, (n1, n2, n2), (n2, 1, 1), (planes, pin[0], pout[0]), cf, inb, pin[1], outb, pout[1]))
        for n1, n2 in ((1024, 1024), (1024, 2048)):
            H = n2 // 2 + 1
            for blocks in (1, 4):
                E = n1 // blocks * H + (16 if blocks > 1 else 0)
                bs = planes * E if blocks > 1 else 0
                yield ('guru2_real r2c f%d %dx%d blocks %d' % (8 * prec, n1, n2, blocks),
                       lambda n1=n1, n2=n2, H=H, blocks=blocks, E=E, bs=bs:
                       eng.plan_create_guru2_real(prec, R2C, (n1, n2, H), (n2, 1, 1), (planes, n1 * n2, E), 1, 0, blocks, bs))
                yield ('guru2_real c2r f%d %dx%d blocks %d' % (8 * prec, n1, n2, blocks),
                       lambda n1=n1, n2=n2, H=H, blocks=blocks, E=E, bs=bs:
                       eng.plan_create_guru2_real(prec, C2R, (n1, H, n2), (n2, 1, 1), (planes, E, n1 * n2), blocks, bs, 1, 0))
        # every other creator, small: strided batched lines (64 lines, blocks laid out as gfft_pack does), one of them truncating
        for n, keep in ((16, 0), (48, 0), (48, 32), (64, 0), (1024, 0)):
            for inb, outb in ((1, 1), (4, 1), (1, 4)):
                yield ('guru %+d f%d n=%d keep=%d blocks %d -> %d' % (FWD, 8 * prec, n, keep, inb, outb),
                       lambda n=n, keep=keep, inb=inb, outb=outb:
                       eng.plan_create_guru(prec, FWD, (n, 1, 1), [(64, n // inb, (keep or n) // outb)], inb, 64 * (n // inb),
                                            outb, 64 * ((keep or n) // outb), keep))
        # ... the padded (3/2-rule) 3-D transform above the size where the workspace schedule starts, complex and real
        for kind in (FWD, BWD):
            yield 'padded c2c %+d f%d 192^3 keep 128^3' % (kind, 8 * prec), lambda kind=kind: eng.plan_create_padded((192,) * 3, (128,) * 3, kind, prec)
        for kind in (R2C, C2R):
            yield 'padded %s f%d 384^3 keep (256, 256, 129)' % ('r2c' if kind == R2C else 'c2r', 8 * prec), \
                lambda kind=kind: eng.plan_create_padded((384,) * 3, (256, 256, 129), kind, prec)
        # ... the eight real-to-real kinds (REDFT00 = 3 ... RODFT11 = 10) on a one-pass logical length and off it
        for n in (16, 17):
            for kind in range(3, 11):
                yield 'r2r kind %d f%d (8, %d)' % (kind, 8 * prec, n), lambda n=n, kind=kind: eng.plan_create_r2r((8, n), (1,), (kind,), prec)
        # ... and one line length per family of plan_line: 2^k, 3 x 2^k, 7-smooth in one pass, small primes (generic), four-step
        # (2^20 and 3 x 2^18), a prime (Bluestein)
        for n in (1024, 768, 896, 1001, 1 << 20, 3 << 18, 1009):
            yield 'c2c %+d f%d (4, %d) axes (1,)' % (FWD, 8 * prec, n), lambda n=n: eng.plan_create((4, n), (4, n), (1,), FWD, prec)


brief = '--brief' in sys.argv[1:]
digest = lambda text: hashlib.sha256(text.encode()).hexdigest()[:12]
default, other = {}, {}
for opt in OPTIONS:
    name = ', '.join('%s = %d' % kv for kv in opt.items()) or 'defaults'
    if not brief:
        print('#### options: %s' % name)
    for k, v in {**DEFAULTS, **opt}.items():
        _lib.set_option(k, v)
    same = 0
    for title, make in requests():
        text = fingerprint(make)
        if default.setdefault(title, text) == text and opt:
            same += 1
        elif brief:
            other.setdefault(title, []).append('%s: %s' % (name, digest(text)) if opt else None)
        else:
            print('== %s\n%s' % (title, text), end='')
    if opt and not brief:
        print('(%d requests as under the defaults)' % same)
for k, v in DEFAULTS.items():
    _lib.set_option(k, v)
if brief:
    # one line per request: its passes under the defaults, the digest of its full text, and the options under which it comes out otherwise
    for title, text in default.items():
        passes = ' + '.join(re.findall(r'pass \d+: (.*), [-0-9.e+]+ bytes', text)) or text.strip()
        print('%s | %s | %s | %s' % (title, passes, digest(text), '; '.join(o for o in other[title] if o) or '-'))
