#!/usr/bin/env python3
"""No GPU needed: proves that two builds of csrc/ carry the same device code -- what a refactor of the kernel files has to show.
For every object (*.o) of both build directories: the gfx950 code object is unbundled from the fat binary, and its .text and
.rodata bytes, its notes (the kernel metadata: VGPRs, LDS, scratch, arguments) and its sorted symbol names must be identical; so
must the symbol names of the host object.  __hip_cuid_<hash> / __hip_gpubin_handle_<hash> hash the source text and are ignored.
usage: codeobj_diff.py <build dir A> <build dir B>   (exit status 1 on any difference; objects in one directory only are listed)"""
import glob, os, re, subprocess, sys, tempfile

LLVM = os.environ.get('LLVM_BIN', '/opt/rocm/llvm/bin')
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'
HASHED = re.compile(r'__hip_(cuid|gpubin_handle)_[0-9a-f]+')


def run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool)] + list(args), check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout


def section(obj, name, tmp):
    out = os.path.join(tmp, 'sec')
    run('llvm-objcopy', '-O', 'binary', '--only-section=' + name, obj, out)
    return open(out, 'rb').read() if os.path.exists(out) else b''


def symbols(obj):
    rows = (l.split() for l in run('llvm-readelf', '--symbols', '--wide', obj).decode().split('\n'))
    return sorted(r[7] for r in rows if len(r) == 8 and r[0].rstrip(':').isdigit() and not HASHED.fullmatch(r[7]))


def facts(obj):
    """what must not move, by name"""
    with tempfile.TemporaryDirectory() as tmp:
        f = {'host symbols': symbols(obj)}
        fat, co = os.path.join(tmp, 'fatbin'), os.path.join(tmp, 'co')
        open(fat, 'wb').write(section(obj, '.hip_fatbin', tmp))
        if os.path.getsize(fat) == 0:
            return f                      # (no device code in this object)
        run('clang-offload-bundler', '--unbundle', '--type=o', '--input=' + fat, '--targets=' + TARGET, '--output=' + co)
        f.update({'.text': section(co, '.text', tmp), '.rodata': section(co, '.rodata', tmp),
                  'notes': run('llvm-readelf', '--notes', co), 'device symbols': symbols(co)})
        return f


a, b = sys.argv[1:3]
names = lambda d: {os.path.basename(p) for p in glob.glob(os.path.join(d, '*.o'))}
bad = 0
for o in sorted(names(a) ^ names(b)):
    print('%-28s only in %s' % (o, a if o in names(a) else b))
    bad += 1
for o in sorted(names(a) & names(b)):
    fa, fb = facts(os.path.join(a, o)), facts(os.path.join(b, o))
    diff = [k for k in fa if fa[k] != fb.get(k)] + [k for k in fb if k not in fa]
    for k in diff:
        if 'symbols' in k:
            print('   %s %s: only in A %s, only in B %s' % (o, k, sorted(set(fa[k]) - set(fb.get(k, [])))[:6], sorted(set(fb.get(k, [])) - set(fa[k]))[:6]))
    size = ', '.join('%s %d B' % (k, len(fa[k])) for k in ('.text', '.rodata') if k in fa)
    print('%-28s %s' % (o, 'DIFFERS: ' + ', '.join(diff) if diff else 'identical (%s, %d device / %d host symbols)'
                        % (size or 'host only', len(fa.get('device symbols', [])), len(fa['host symbols']))))
    bad += bool(diff)
print('%d objects compared, %s' % (len(names(a) & names(b)), 'all identical' if not bad else '%d DIFFER or are unpaired' % bad))
sys.exit(1 if bad else 0)
