#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds, instruction for instruction: tools/kernel_diff.py <build dir A> <build dir B>

For every *.o of a directory the gfx950 code object is extracted (llvm-objdump --offloading) and disassembled without raw bytes and
addresses; the `//` address comments are stripped and the text is split per function symbol.  The resource metadata of every kernel
comes from the code object's notes (llvm-readelf --notes).  Kernels are matched by symbol over the WHOLE directory, so a kernel may move
from one source file to another between the builds.  Reported: symbols that exist on one side only, and symbols whose instructions or
metadata differ; the exit status is non-zero if there are any.  This is the check of a refactor that must not change generated code.
Needs nothing but the ROCm LLVM tools (LLVM_BIN, default /opt/rocm/llvm/bin)."""
import difflib
import glob
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get('LLVM_BIN', '/opt/rocm/llvm/bin')
META = ('.vgpr_count', '.agpr_count', '.sgpr_count', '.vgpr_spill_count', '.sgpr_spill_count', '.group_segment_fixed_size',
        '.private_segment_fixed_size', '.max_flat_workgroup_size', '.kernarg_segment_size')


def run(tool, *args, cwd=None):
    return subprocess.run([os.path.join(LLVM, tool)] + list(args), cwd=cwd, check=True, capture_output=True, text=True).stdout


def code_objects(obj, tmp):
    """the gfx950 code objects bundled in one host object"""
    d = tempfile.mkdtemp(dir=tmp)
    os.symlink(os.path.abspath(obj), os.path.join(d, os.path.basename(obj)))      # (the bundles are written next to the path given)
    run('llvm-objdump', '--offloading', os.path.basename(obj), cwd=d)
    return [f for f in glob.glob(os.path.join(d, '*gfx950*')) if os.path.getsize(f)]


def functions(co):
    """symbol -> instruction text"""
    out, cur = {}, None
    for line in run('llvm-objdump', '-d', '--no-show-raw-insn', '--no-leading-addr', co).splitlines():
        m = re.match(r'^(?:[0-9a-f]+ )?<(.+)>:$', line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip() not in ('', '...'):      # '...': zero bytes skipped (padding behind a file's last function)
            cur.append(line.split('//')[0].rstrip())
    return {k: '\n'.join(v) for k, v in out.items()}


def metadata(co):
    """kernel symbol -> {field: value} from the amdhsa.kernels list of the notes"""
    out, cur = {}, None
    for line in run('llvm-readelf', '--notes', co).splitlines():
        m = re.match(r'^  (- | {2})(\.\w+):\s*(.*)$', line)      # the list's own level only (arguments are nested deeper)
        if not m:
            continue
        if m.group(1) == '- ':
            cur = {}
        if cur is None:
            continue
        if m.group(2) == '.name':
            out[m.group(3)] = cur
        elif m.group(2) in META:
            cur[m.group(2)] = m.group(3)
    return out


def build(directory, tmp):
    """symbol -> set of (file-independent) (instructions, metadata) over every object of the directory"""
    syms = {}
    objs = sorted(glob.glob(os.path.join(directory, '*.o')))
    if not objs:
        sys.exit(f'{directory}: no objects')
    for obj in objs:
        for co in code_objects(obj, tmp):
            meta = metadata(co)
            for name, text in functions(co).items():
                syms.setdefault(name, set()).add((text, tuple(sorted(meta.get(name, {}).items()))))
    return syms


def main(a_dir, b_dir):
    with tempfile.TemporaryDirectory() as tmp:
        a, b = build(a_dir, tmp), build(b_dir, tmp)
    bad = 0
    for name in sorted(set(a) - set(b)):
        bad += 1
        print(f'only in {a_dir}: {name}')
    for name in sorted(set(b) - set(a)):
        bad += 1
        print(f'only in {b_dir}: {name}')
    for name in sorted(set(a) & set(b)):
        if a[name] == b[name]:
            continue
        bad += 1
        (ta, ma), (tb, mb) = sorted(a[name])[0], sorted(b[name])[0]
        if ma != mb:
            print(f'metadata differs: {name}\n  {dict(ma)}\n  {dict(mb)}')
        if ta != tb:
            d = list(difflib.unified_diff(ta.splitlines(), tb.splitlines(), a_dir, b_dir, lineterm='', n=1))
            print(f'instructions differ: {name} ({len(ta.splitlines())} / {len(tb.splitlines())} lines)')
            print('\n'.join('  ' + l for l in d[:40]))
        if len(a[name]) != len(b[name]):
            print(f'copies differ: {name} has {len(a[name])} / {len(b[name])} distinct bodies')
    def kernels(syms):      # symbols that came with every metadata field: the kernels
        return {n for n, v in syms.items() if all(len(m) == len(META) for _, m in v)}
    ka, kb = kernels(a), kernels(b)
    print(f'{len(ka & kb)} kernels compared (instructions and metadata) and {len((set(a) & set(b)) - (ka & kb))} other function symbols '
          f'(instructions), {bad} differ or are missing')
    if not ka or not kb:      # the notes did not parse: nothing above compared any metadata
        print('no kernel metadata found in ' + (a_dir if not ka else b_dir))
        return 2
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
