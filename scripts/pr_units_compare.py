#!/usr/bin/env python3
"""Same device code before and after moving kernels between units (no GPU needed).

    scripts/pr_units_compare.py PARENT_TREE [--parent-units mr_pagerank.hip]
                                [--units mr_pagerank.hip mr_pr_plan.hip ...] > kernel_resources_compare.txt

Compiles the named units of both trees device-only with the Makefile's FLAGS plus
-Rpass-analysis=kernel-resource-usage (a plain gfx950 ELF each) and compares, kernel by kernel:
the set of demangled names over each side's units together, the remark's resource lines, and the
bytes of the kernel's function symbol in .text.  Exit status 1 when anything differs.
"""
import argparse
import difflib
import hashlib
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ['mr_pagerank.hip', 'mr_pr_plan.hip', 'mr_pr_launch.hip', 'mr_pr_walk.hip', 'mr_pr_fxb.hip',
         'mr_pr_tile_cold.hip']
COLS = ['TotalSGPRs', 'VGPRs', 'AGPRs', 'ScratchSize [bytes/lane]', 'LDS Size [bytes/block]', 'Occupancy [waves/SIMD]']
ROCM = os.environ.get('ROCM_PATH', '/opt/rocm')
TOOLS = os.pathsep.join([os.path.join(ROCM, 'lib', 'llvm', 'bin'), os.path.join(ROCM, 'llvm', 'bin'), os.environ.get('PATH', '')])


def demangle(names):
    """demangled names (the mangled ones where no demangler is installed: they compare as well)"""
    tool = shutil.which('llvm-cxxfilt', path=TOOLS) or shutil.which('c++filt', path=TOOLS)
    if not tool or not names:
        return list(names)
    return subprocess.run([tool] + list(names), check=True, capture_output=True, text=True).stdout.splitlines()


def make_var(csrc, var):
    return subprocess.run(['make', '-s', '-C', csrc, '--no-print-directory', '--eval', 'pv: ; @echo $(%s)' % var, 'pv'],
                          check=True, capture_output=True, text=True).stdout.split()


def elf_kernels(path):
    """{mangled name: bytes of its function symbol} for every symbol NAME that has a NAME.kd descriptor"""
    b = open(path, 'rb').read()
    shoff, = struct.unpack_from('<Q', b, 0x28)
    shentsize, shnum = struct.unpack_from('<HH', b, 0x3A)
    secs = [struct.unpack_from('<IIQQQQIIQQ', b, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for s in secs:
        if s[1] != 2:   # SHT_SYMTAB
            continue
        stroff = secs[s[6]][4]
        syms = {}
        for o in range(s[4], s[4] + s[5], 24):
            name, _info, _other, shndx, value, size = struct.unpack_from('<IBBHQQ', b, o)
            syms[b[stroff + name:b.index(b'\0', stroff + name)].decode()] = (shndx, value, size)
        for nm, (shndx, value, size) in syms.items():
            if nm + '.kd' in syms:
                sec = secs[shndx]
                off = sec[4] + value - sec[3]
                out[nm] = b[off:off + size]
    return out


def compile_units(tree, units, tmp, tag):
    csrc = os.path.join(tree, 'microrank_amd', 'csrc')
    hipcc, flags = make_var(csrc, 'HIPCC')[0], make_var(csrc, 'FLAGS')
    kernels = {}   # demangled name -> (unit, resources, code bytes, elf, mangled)
    twice = []
    for u in units:
        elf = os.path.join(tmp, '%s_%s.elf' % (tag, u))
        r = subprocess.run([hipcc] + flags + ['--cuda-device-only', '--no-gpu-bundle-output',
                                              '-Rpass-analysis=kernel-resource-usage', '-c', u, '-o', elf],
                           cwd=csrc, check=True, capture_output=True, text=True)
        res, cur = {}, None
        for line in r.stderr.splitlines():
            m = re.search(r'remark:\s+(.*?):\s+(\S+)\s+\[-Rpass-analysis', line)
            if not m:
                continue
            if m.group(1) == 'Function Name':
                cur = res.setdefault(m.group(2), {})
            elif cur is not None:
                cur[m.group(1)] = m.group(2)
        code = elf_kernels(elf)
        names = sorted(code)
        for mangled, d in zip(names, demangle(names)):
            d = d.replace('(anonymous namespace)::', '')
            d = re.sub(r'^void ', '', d)
            if d in kernels:
                twice.append('%s: %s and %s' % (d, kernels[d][0], u))
            kernels[d] = (u, res.get(mangled, {}), code[mangled], elf, mangled)
    return kernels, twice


def disasm(elf, mangled):
    t = subprocess.run([shutil.which('llvm-objdump', path=TOOLS), '-d', '--no-show-raw-insn', '--no-leading-addr',
                        '--disassemble-symbols=' + mangled, elf], capture_output=True, text=True).stdout
    return t.splitlines()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('parent')
    ap.add_argument('--parent-units', nargs='+', default=['mr_pagerank.hip'])
    ap.add_argument('--units', nargs='+', default=UNITS)
    a = ap.parse_args()
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        old, old2 = compile_units(a.parent, a.parent_units, tmp, 'parent')
        new, new2 = compile_units(HERE, a.units, tmp, 'tree')
        print('# parent: %d kernels in %s; this tree: %d kernels in %s' % (len(old), ' '.join(a.parent_units), len(new),
                                                                        ' '.join(a.units)))
        for what, names in (('only in the parent', sorted(set(old) - set(new))),
                            ('only in this tree', sorted(set(new) - set(old))),
                            ('instantiated twice', old2 + new2)):
            print('# %s: %s' % (what, '; '.join(names) if names else 'none'))
            bad += len(names)
        print(' | '.join(['kernel', 'unit'] + COLS + ['resources against the parent', 'code bytes', 'sha256[:12]',
                                                      'code against the parent']))
        diffs = []
        for k in sorted(set(old) & set(new)):
            u, res, code, elf, mangled = new[k]
            same_r = all(res.get(c) is not None and res.get(c) == old[k][1].get(c) for c in COLS)
            same_c = code == old[k][2]
            bad += (not same_r) + (not same_c)
            print(' | '.join([k.split('(')[0], u] + [str(res.get(c)) for c in COLS] +
                             ['same' if same_r else 'DIFFERENT (parent: %s)' % ' '.join(str(old[k][1].get(c)) for c in COLS),
                              str(len(code)), hashlib.sha256(code).hexdigest()[:12], 'same' if same_c else 'DIFFERENT']))
            if not same_c:
                diffs.append((k, list(difflib.unified_diff(disasm(old[k][3], old[k][4]), disasm(elf, mangled), 'parent',
                                                           'tree', lineterm='', n=2))))
        for k, d in diffs:
            print('\n# disassembly diff of %s (%d lines)' % (k, len(d)))
            print('\n'.join(d[:400]))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
