#!/usr/bin/env python3
"""Does a source-level refactor leave the GPU machine code alone?  CPU only.

    python tools/kernel_isa_diff.py old.co new1.co [new2.co ...]

Each argument is a gfx950 code object, i.e. a .hip file compiled with the Makefile's flags plus
`--cuda-device-only --no-gpu-bundle-output -c`.  The kernels of `old.co` are compared with the union of the kernels of
the new objects (one old translation unit split into several, or the other way round with the roles swapped):

  * the set of kernel symbols must be the same -- none missing, none added, none in two new objects;
  * per kernel, the `llvm-objdump -d` instruction stream (mnemonic, operands and encoding; the addresses are dropped,
    branch targets print relative to their symbol) must be the same;
  * per kernel, the metadata of `llvm-readelf --notes` listed in FIELDS must be the same.

Device functions that were not inlined are compared like kernels (instruction stream only).  One kind of difference is
reported apart, as "rodata-relative only": an instruction pair that differs in nothing but a 32-bit literal right
after an s_getpc_b64 -- the pc-relative address of a .rodata object, which moves when the code object's layout does.
(The pattern alone decides: the tool does not resolve the address, so it does not prove that the target lies in
.rodata.  It reports every such kernel by name; whoever claims the exception looks at the listed instructions.)
Exit status 0: identical (such literals aside); 1: anything else.
"""
import argparse
import os
import re
import subprocess
import sys

FIELDS = ('.vgpr_count', '.agpr_count', '.sgpr_count', '.group_segment_fixed_size', '.private_segment_fixed_size',
          '.kernarg_segment_size', '.max_flat_workgroup_size', '.vgpr_spill_count', '.sgpr_spill_count')


def tool(name):
    root = os.environ.get('ROCM_PATH', '/opt/rocm')
    p = os.path.join(root, 'llvm', 'bin', name)
    return p if os.path.exists(p) else name


def run(cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def kernel_metadata(path):
    """{kernel name: {field: value}} from the amdhsa.kernels list of the metadata note."""
    kernels = []
    for line in run([tool('llvm-readelf'), '--notes', path]).splitlines():
        m = re.match(r'^  (- | {2})(\.\w+):\s*(.*)$', line)      # a kernel's own keys sit at this depth; .args lie deeper
        if not m:
            continue
        if m.group(1) == '- ':
            kernels.append({})
        if kernels:
            kernels[-1][m.group(2)] = m.group(3).strip()
    return {k['.name']: k for k in kernels if '.name' in k}


def disassembly(path):
    """{function symbol: [(text, encoding), ...]} of .text."""
    out, cur = {}, None
    for line in run([tool('llvm-objdump'), '-d', path]).splitlines():
        m = re.match(r'^[0-9a-fA-F]+ <(.+)>:$', line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None or not line.startswith('\t'):
            continue
        text, _, tail = line.partition('//')
        if text.strip() == '...':                                  # objdump's ellipsis over a run of zero bytes
            continue
        enc = re.sub(r'^\s*[0-9A-Fa-f]+:\s*', '', tail)           # drop the address, keep the encoding and the <sym+off>
        cur.append((' '.join(text.split()), ' '.join(enc.split())))
    for ins in out.values():       # the s_nop run that pads a function to the next one's alignment: the last function of
        while ins and ins[-1][0] == 's_nop 0':     # .text has none, and which function is last is not the kernel's business
            ins.pop()
    return out


def compare_streams(a, b):
    """-> (hard differences, rodata-relative literal differences), as lists of instruction indices."""
    if len(a) != len(b):
        return [-1], []
    hard, soft = [], []
    getpc_at = -10
    for i, (x, y) in enumerate(zip(a, b)):
        if x[0].startswith('s_getpc_b64'):
            getpc_at = i
        if x == y:
            continue
        # s_getpc_b64 ; s_add_u32 lo, lo, LITERAL ; s_addc_u32 hi, hi, LITERAL: same opcode and registers, other literal
        strip = lambda t: re.sub(r'(0x[0-9a-fA-F]+|-?\d+)$', '', t[0])
        if i - getpc_at <= 2 and re.match(r's_addc?_u32 ', x[0]) and strip(x) == strip(y):
            soft.append(i)
        else:
            hard.append(i)
    return hard, soft


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('old')
    ap.add_argument('new', nargs='+')
    ap.add_argument('-v', '--verbose', action='store_true', help='list every kernel, not only the differing ones')
    args = ap.parse_args()

    old_meta, old_dis = kernel_metadata(args.old), disassembly(args.old)
    new_meta, new_dis, owner, bad = {}, {}, {}, 0
    for path in args.new:
        meta, dis = kernel_metadata(path), disassembly(path)
        for k in meta:
            if k in new_meta:
                print(f'DUPLICATE kernel {k}: in {owner[k]} and in {path}')
                bad += 1
            owner[k] = path
        new_meta.update(meta)
        for s, ins in dis.items():
            if s in new_dis and new_dis[s] != ins:
                print(f'DUPLICATE function {s} with different code: in {owner.get(s, "?")} and in {path}')
                bad += 1
            owner.setdefault(s, path)
            new_dis[s] = ins
    for k in sorted(set(old_meta) - set(new_meta)):
        print(f'MISSING kernel {k}')
        bad += 1
    for k in sorted(set(new_meta) - set(old_meta)):
        print(f'ADDED kernel {k} ({owner[k]})')
        bad += 1
    for s in sorted((set(old_dis) ^ set(new_dis)) - set(old_meta) - set(new_meta)):
        print(f'{"MISSING" if s in old_dis else "ADDED"} device function {s}')
        bad += 1

    n_same = n_soft = n_ins = 0
    for s in sorted(set(old_dis) & set(new_dis)):
        hard, soft = compare_streams(old_dis[s], new_dis[s])
        n_ins += len(old_dis[s])
        fields = []
        if s in old_meta and s in new_meta:
            fields = [f for f in FIELDS if old_meta[s].get(f) != new_meta[s].get(f)]
        if hard or fields:
            bad += 1
            what = 'length differs' if hard == [-1] else f'{len(hard)} instructions differ (first at #{hard[0]})' if hard else ''
            print(f'DIFFERENT {s} ({owner[s]}): {what} {" ".join(f"{f}: {old_meta[s].get(f)} -> {new_meta[s].get(f)}" for f in fields)}')
            if hard and hard != [-1]:
                for i in hard[:4]:
                    print(f'    #{i}: {old_dis[s][i]}\n     -> {new_dis[s][i]}')
        elif soft:
            n_soft += 1
            print(f'rodata-relative only: {s} ({owner[s]}): literals at instructions {soft}')
        else:
            n_same += 1
            if args.verbose:
                print(f'same {s} ({owner[s]}, {len(old_dis[s])} instructions)')
    print(f'{len(old_meta)} kernels in {args.old}, {len(new_meta)} in {len(args.new)} new object(s); '
          f'{n_same} functions identical ({n_ins} instructions compared), {n_soft} rodata-relative only, {bad} problems')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
