#!/usr/bin/env python3
"""Development aid: per-kernel resources and instruction counts of the SegNet kernel files from their gfx950 device
assembly, for two source trees side by side (a refactor must not move them).  For each tree:
    for f in spa_segnet spa_segnet_bf16 spa_segnet_f16x3 spa_segnet_train spa_segnet_train_bf16 spa_segnet_train_f16x3; do
        hipcc --offload-arch=gfx950 <the Makefile's CXXFLAGS> --cuda-device-only -S \\
              -Rpass-analysis=kernel-resource-usage $f.hip -o DIR/$f.s 2> DIR/$f.rpass; done
then  python tools/segnet_isa_table.py OLD_DIR NEW_DIR > profiles/segnet_refactor_isa.md
Kernels are matched by demangled template name (arguments dropped: a shared struct renames them); RENAMED maps the
small kernels that were merged.  Counted per kernel: every v_mfma_*, ds_*, global_* / buffer_* / flat_*, s_barrier and
floating-point VALU mnemonic; scalar and integer instructions are free to differ.  Exit status 1 if a counted
mnemonic, the LDS size, scratch or spills differ."""
import collections, os, re, subprocess, sys

FILES = ['spa_segnet', 'spa_segnet_bf16', 'spa_segnet_f16x3', 'spa_segnet_train', 'spa_segnet_train_bf16',
         'spa_segnet_train_f16x3']
RENAMED = {'k_segnet_wpack64_bf16': 'k_sg_bf16_wpack64', 'k_sgb_wpack64': 'k_sg_bf16_wpack64',
           'k_segnet_wpack1_bf16': 'k_sg_bf16_wpack1', 'k_sgb_wpack1': 'k_sg_bf16_wpack1',
           'k_sgx_wpack64': 'k_sg_split_wpack64', 'k_sgh_wpack64': 'k_sg_split_wpack64',
           'k_sgx_wpack1': 'k_sg_split_wpack1', 'k_sgh_wpack1': 'k_sg_split_wpack1',
           'k_sgx_scale': 'k_sg_scale', 'k_sgh_scale': 'k_sg_scale',
           'k_sgt_bnstat': 'k_sg_bnstat', 'k_sgb_bnstat': 'k_sg_bnstat', 'k_sgh_bnstat': 'k_sg_bnstat',
           'k_sgt_wsum': 'k_sg_wsum', 'k_sgb_wsum': 'k_sg_wsum', 'k_sgh_wsum': 'k_sg_wsum'}
FP = re.compile(r'^v_\w*_(f32|f16|f64|bf16)(_|$)|^v_cvt_|^v_pk_|^v_exp_|^v_rcp_|^v_div_|^v_ldexp_|^v_fma')
META = ['.vgpr_count', '.agpr_count', '.sgpr_count', '.group_segment_fixed_size', '.private_segment_fixed_size',
        '.vgpr_spill_count']


def counted(mn):
    return (mn.startswith(('v_mfma_', 'ds_', 'global_', 'buffer_', 'flat_')) or mn == 's_barrier' or bool(FP.match(mn)))


def demangle(names):
    out = subprocess.run(['c++filt'] + names, capture_output=True, text=True, check=True)
    res = {}
    for m, d in zip(names, out.stdout.split('\n')):
        d = re.sub(r'^void ', '', d)
        d = re.sub(r'\(anonymous namespace\)::', '', d)
        i = d.find('(')                                    # drop the arguments, keep the template arguments
        base = d[:i] if i > 0 else d
        name = base.split('<')[0]
        res[m] = RENAMED.get(name, name) + base[len(name):]
    return res


def load(d, f):
    text = open(os.path.join(d, f + '.s')).read().split('\n')
    kern, cur = {}, None
    for line in text:                                      # the metadata list at the end of the file
        s = line.strip()
        if s.startswith('- .agpr_count') or s.startswith('- .args'):
            cur = {}
            s = s[2:]
        if cur is not None:
            k = s.split(':')[0]
            if k in META:
                cur[k] = int(s.split(':')[1])
            elif k == '.name':
                kern[s.split(':')[1].strip()] = cur
    for m in kern:
        kern[m]['ins'] = collections.Counter()
    cur = None
    for line in text:
        if line.split(':')[0] in kern and not line.startswith(('\t', ' ')):
            cur = kern[line.split(':')[0]]['ins']
        elif line.startswith('.Lfunc_end'):
            cur = None
        elif cur is not None and line.startswith('\t') and not line.startswith('\t.'):
            mn = line.split()[0]
            if counted(mn):
                cur[mn] += 1
    occ, name = {}, None
    for line in open(os.path.join(d, f + '.rpass')):
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = m.group(1)
        m = re.search(r'Occupancy \[waves/SIMD\]: (\d+)', line)
        if m and name:
            occ[name] = int(m.group(1))
    names = demangle(sorted(kern))
    return {names[m]: dict(kern[m], occ=occ.get(m)) for m in kern}


def cls(ins, pre):
    return sum(v for k, v in ins.items() if k.startswith(pre))


def row(k):
    if k is None:
        return ['-'] * 11
    i = k['ins']
    fp = sum(v for m, v in i.items() if FP.match(m) and not m.startswith('v_mfma_'))
    return [k.get('.vgpr_count'), k.get('.agpr_count', 0), k.get('.sgpr_count'), k.get('.group_segment_fixed_size'),
            k.get('.private_segment_fixed_size'), k.get('.vgpr_spill_count'), k['occ'], cls(i, 'v_mfma_'), cls(i, 'ds_'),
            cls(i, 'global_') + cls(i, 'buffer_') + cls(i, 'flat_'), '%d / %d' % (i['s_barrier'], fp)]


def main():
    old_dir, new_dir = sys.argv[1:3]
    bad = 0
    print('# SegNet kernels before and after sharing spa_segnet_dev.h: resources and counted instructions\n')
    print('Made by tools/segnet_isa_table.py (its docstring has the compile command).  Columns, old -> new where they')
    print('differ: VGPR, AGPR, SGPR, LDS bytes, scratch bytes, spilled VGPRs, occupancy [waves/SIMD], v_mfma_*, ds_*,')
    print('global_* + buffer_* + flat_*, s_barrier / floating-point VALU instructions.  "mnemonics" lists every counted')
    print('mnemonic whose count differs (none: all equal).\n')
    for f in FILES:
        old, new = load(old_dir, f), load(new_dir, f)
        print('## %s.hip\n' % f)
        print('| kernel | vgpr | agpr | sgpr | lds | scratch | spills | occ | mfma | ds | global | barrier / fp | mnemonics |')
        print('|---|---|---|---|---|---|---|---|---|---|---|---|---|')
        for name in sorted(set(old) | set(new)):
            o, n = old.get(name), new.get(name)
            ro, rn = row(o), row(n)
            cells = [str(a) if a == b else '%s -> %s' % (a, b) for a, b in zip(ro, rn)]
            diff = ''
            if o and n:
                ms = sorted(set(o['ins']) | set(n['ins']))
                diff = ', '.join('%s %d -> %d' % (m, o['ins'][m], n['ins'][m]) for m in ms if o['ins'][m] != n['ins'][m])
                if diff or any(ro[j] != rn[j] for j in (3, 4, 5)):
                    bad = 1
            print('| `%s` | %s | %s |' % (name, ' | '.join(cells), diff or ('none' if o and n else 'only in one tree')))
        print()
    return bad


if __name__ == '__main__':
    sys.exit(main())
