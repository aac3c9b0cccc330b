#!/usr/bin/env python3
"""Are kernels of one tree the instruction streams of another tree's?  Compiles the named csrc/*.hip of both trees for gfx950 with
-save-temps (the flags of csrc/build.sh, as tools/kernel_resources.py does) and compares, kernel by kernel, the instruction lines of
the generated assembly -- comments and the numbering of local labels dropped, nothing else: registers, immediates and argument offsets
all count.  Kernels are paired by demangled name; PAIRS below maps a kernel that became a template instantiation to its old name.
CPU only (hipcc cross-compiles).

    git worktree add /tmp/parent HEAD~1
    python tools/kernel_stream_diff.py /tmp/parent . small_kernels train_kernels > profiles/<what>_kernel_streams.txt"""
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join('image-super-resolution-via-iterative-refinement_amd', 'csrc')
FLAGS = '--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-function -save-temps'.split()
# old demangled name (up to its argument list) -> new one
PAIRS = {
    'sr3::k_gn_finalize': 'void sr3::k_gn_finalize<false>',
    'void sr3::k_rows_fold<true>': 'void sr3::k_rows_fold<true, false>',
    'void sr3::k_rows_fold<false>': 'void sr3::k_rows_fold<false, false>',
    'sr3::k_gn_bwd_group': 'void sr3::k_gn_bwd_group<false>',
    'sr3::k_part_colsum': 'void sr3::k_part_colsum<false>',
    'sr3::k_gn_bwd_apply': 'void sr3::k_gn_bwd_apply<float const* restrict>',
}


def streams(tree, base):
    """{demangled kernel name up to '(': [instruction lines]} of one source file of one tree"""
    tmp = tempfile.mkdtemp(prefix='sr3_streams_')
    src = os.path.join(os.path.abspath(tree), CSRC, base + '.hip')
    subprocess.run(['/opt/rocm/bin/hipcc'] + FLAGS + ['-c', src, '-o', os.path.join(tmp, base + '.o')], cwd=tmp, check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = open(os.path.join(tmp, base + '-hip-amdgcn-amd-amdhsa-gfx950.s')).read()
    names = re.findall(r'\.amdhsa_kernel (\S+)', asm)
    dem = subprocess.run(['c++filt'], input='\n'.join(names).encode(), stdout=subprocess.PIPE).stdout.decode().split('\n')
    out = {}
    for name, d in zip(names, dem):
        body = re.search(r'^' + re.escape(name) + r':[^\n]*\n(.*?)^\.Lfunc_end\d+:', asm, re.S | re.M).group(1)
        ins = []
        for line in body.split('\n'):
            line = re.sub(r';.*', '', line).strip()
            if line and not line.startswith('.'):
                ins.append(re.sub(r'\.LBB\d+_', '.LBB_', line))
            elif re.match(r'\.LBB\d+_\d+:', line):
                ins.append(re.sub(r'\.LBB\d+_', '.LBB_', line))
        out[re.sub(r'\(.*', '', d)] = ins
    return out


def main():
    old_tree, new_tree, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    print('file              instr (old)  instr (new)  differing lines  kernel (old name -> new name where it changed)')
    total = same = 0
    for base in files:
        old, new = streams(old_tree, base), streams(new_tree, base)
        for k in sorted(old):
            k2 = PAIRS.get(k, k)
            if k2 not in new:
                print('%-17s %11d %12s %16s  %s' % (base, len(old[k]), '-', '-', k + '  (gone)'))
                continue
            a, b = old[k], new[k2]
            nd = sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b))
            total += 1
            same += nd == 0
            label = k if k2 == k else '%s -> %s' % (k, k2)
            print('%-17s %11d %12d %16d  %s' % (base, len(a), len(b), nd, label.replace('void ', '').replace('sr3::', '')))
        for k in sorted(set(new) - {PAIRS.get(o, o) for o in old}):
            print('%-17s %11s %12d %16s  %s' % (base, '-', len(new[k]), '-', k.replace('void ', '').replace('sr3::', '') + '  (new)'))
    print('\n%d of %d kernels present in both trees have identical instruction streams' % (same, total))


if __name__ == '__main__':
    main()
