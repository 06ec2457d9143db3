#!/usr/bin/env python3
"""Build-time check: the Gram ring's loads stay in flight across an iteration.

    python scripts/check_ring_waits.py [--arch=gfx950] exp-trmf-nips16_amd/build/f32/unit_gram.o [unit_split.o ...]   (objects of the build)
    python scripts/check_ring_waits.py some_kernels.s                                              (hipcc -S output)

gram_ring (csrc/gram_kernels.hpp) consumes a group of four gathered factor rows with NT (NT + 1) / 2 MFMAs and re-requests the
group's slot at once; its loop is written so that the compiler's `s_waitcnt vmcnt(N)` before each group waits for THAT group's
loads and leaves the later groups' loads outstanding.  That property lives in the compiled code only: an instruction order in
the loop's prologue that differs from the loop body's makes the waitcnt pass merge two load orders at the loop header into one
vmcnt(0), and the kernel then drains all its gathers every iteration without any test noticing (the results are the same).
This tool reads the device code the build produced and fails unless, in every ring loop,

  * at most one group's worth of 16x16x4 MFMAs, NT (NT + 1) / 2, lies between two consecutive `s_waitcnt vmcnt`, and
  * no `s_waitcnt vmcnt(0)` stands anywhere between the loop header and the loop's last MFMAs.

A ring loop is a loop (a label and a later branch back to it) with basic blocks that hold 16x16x4 MFMAs; it is judged as one
sequence in program order from its header to its last MFMA, blocks without MFMAs included (the summary shows the block boundaries as
||); only `s_waitcnt` and `v_mfma` instructions are judged.  Kernels without such a loop are ignored.  NT is the kernel's first integer template argument
(all ring kernels have it there); without one, a quarter of the loop's MFMAs (the ring is four groups deep).
Instantiations that are known not to meet the rule go into ALLOW with the reason."""
import os
import re
import subprocess
import sys
import tempfile

LLVM_BIN = os.environ.get('LLVM_BIN', '/opt/rocm/lib/llvm/bin')
ARCH = 'gfx950'                                 # --arch=<name> on the command line (the Makefile passes its own)
RING_DEPTH = 4
# pretty kernel name (as printed in the summary) -> reason
ALLOW = {}

_FUNC = re.compile(r'^(?:[0-9a-fA-F]+\s+)?<?([A-Za-z_.$][\w.$]*)>?:')
_VMCNT = re.compile(r'vmcnt\((\d+)\)')


def pretty(name):
    """_ZN4trmf18fsolve_quad_kernelILi3ELi40EEEv... -> fsolve_quad_kernel<3,40>; other names are returned as they are."""
    m = re.match(r'_ZN4trmf(\d+)', name)
    if not m:
        return name
    start = m.end()
    base = name[start:start + int(m.group(1))]
    rest = name[start + int(m.group(1)):]
    args = []
    if rest.startswith('I'):
        rest = rest[1:]
        while True:
            a = re.match(r'L([ibjlm])(n?)(\d+)E', rest)
            if not a:
                break
            v = ('-' if a.group(2) else '') + a.group(3)
            args.append({'0': 'false', '1': 'true'}.get(v, v) if a.group(1) == 'b' else v)
            rest = rest[a.end():]
    return base + ('<' + ','.join(args) + '>' if args else '')


def first_int_arg(name):
    m = re.search(r'IL[ijlm](\d+)E', name)
    return int(m.group(1)) if m else None


def parse(text):
    """ISA text (hipcc -S or llvm-objdump -d --symbolize-operands) -> {kernel: [item]}; an item is ('label', name),
    ('branch', target), ('wait', N) for an s_waitcnt with a vmcnt field, ('mfma',) for a 16x16x4 MFMA, ('other_mfma',)."""
    kernels, cur = {}, None
    for raw in text.splitlines():
        line = raw.split(';', 1)[0].split('//', 1)[0].rstrip()
        if not line.strip():
            continue
        m = _FUNC.match(line)
        if m:
            name = m.group(1)
            if name.startswith('.L') or re.fullmatch(r'L\d+', name):
                if cur is not None:
                    cur.append(('label', name))
            elif name.startswith('.') or name.startswith('$'):
                pass
            else:
                cur = kernels.setdefault(name, [])
            continue
        if cur is None:
            continue
        tok = line.split()
        if tok and re.fullmatch(r'[0-9a-fA-F]+:', tok[0]):      # an address column
            tok = tok[1:]
        if not tok or tok[0].startswith('.'):
            continue
        op = tok[0]
        if op.startswith('s_cbranch') or op == 's_branch':
            cur.append(('branch', tok[-1].rstrip(',')))
        elif op == 's_waitcnt':
            w = _VMCNT.search(line)
            if w:
                cur.append(('wait', int(w.group(1))))
        elif op.startswith('v_mfma'):
            cur.append(('mfma',) if '16x16x4' in op else ('other_mfma',))
        elif op in ('s_endpgm', 's_setpc_b64'):
            cur.append(('branch', None))
    return kernels


def ring_loops(items):
    """The ring loops of one kernel: for every innermost loop that holds 16x16x4 MFMAs, the list of its basic blocks in program order from
    the loop header to the block of its last such MFMA; a block is the list of its events [('wait', N) | ('mfma',)].  Blocks without MFMAs
    (the joins behind a skipped group, for instance) are kept: a wait there stands in front of the following groups all the same."""
    pos = {}
    for i, it in enumerate(items):
        if it[0] == 'label':
            pos[it[1]] = i
    spans = []
    for i, it in enumerate(items):
        if it[0] == 'branch' and it[1] in pos and pos[it[1]] < i:
            spans.append((pos[it[1]], i))
    spans = [s for s in spans if any(items[j] == ('mfma',) for j in range(s[0], s[1]))]
    inner = [s for s in spans if not any(o != s and s[0] <= o[0] and o[1] <= s[1] for o in spans)]
    loops = []
    for a, b in sorted(set(inner)):
        blocks, blk = [], []
        for it in items[a:b + 1]:
            if it[0] in ('label', 'branch'):
                blocks.append(blk)
                blk = []
            elif it[0] in ('wait', 'mfma'):
                blk.append(it)
        blocks.append(blk)
        last = max(i for i, blk in enumerate(blocks) if ('mfma',) in blk)
        loops.append([blk for blk in blocks[:last + 1] if blk])
    return loops


def judge(blocks, group):
    """-> (summary text, list of violations) of one ring loop.  The loop is judged as ONE sequence in program order (the block
    boundaries are only shown, as ||): the MFMAs between two consecutive waits are at most a group, and no vmcnt(0) stands anywhere
    in front of the loop's last MFMAs -- not in another block, and not with a second wait behind it either."""
    parts, bad = [], []
    run, zero_seen = 0, False                    # MFMAs since the last wait (across blocks); a vmcnt(0) so far
    for blk in blocks:
        words, shown = [], 0                     # shown: MFMAs of this block not yet written out
        for ev in blk:
            if ev[0] == 'mfma':
                run += 1
                shown += 1
                if zero_seen:
                    bad.append('vmcnt(0) in front of MFMAs: the ring drains its gathers')
                if run == group + 1:
                    bad.append('more than %d MFMAs (a group) behind one wait' % group)
                continue
            if shown:
                words.append('M%d' % shown)
            words.append('[%d]' % ev[1])
            run, shown = 0, 0
            zero_seen = zero_seen or ev[1] == 0
        if shown:
            words.append('M%d' % shown)
        parts.append(' '.join(words))
    return ' || '.join(parts), sorted(set(bad))


def check_text(text):
    """-> list of (kernel, summary, violations, allowed reason or None) for every kernel with a ring loop."""
    out = []
    for name, items in parse(text).items():
        loops = ring_loops(items)
        if not loops:
            continue
        nt = first_int_arg(name)
        short = pretty(name)
        for blocks in loops:
            n_mfma = sum(1 for blk in blocks for e in blk if e == ('mfma',))
            group = nt * (nt + 1) // 2 if nt else max(1, n_mfma // RING_DEPTH)
            summary, bad = judge(blocks, group)
            out.append((short, summary, bad, ALLOW.get(short)))
    return out


def device_isa(path):
    """The device ISA of a file: objects of the build are unbundled and disassembled, anything else is read as text."""
    if not path.endswith(('.o', '.co', '.hsaco')):
        return open(path, errors='replace').read()
    with tempfile.TemporaryDirectory() as tmp:
        co = path
        if path.endswith('.o'):                  # host object: the device code objects are a bundle in the .hip_fatbin section
            fb, co = os.path.join(tmp, 'device.hipfb'), os.path.join(tmp, 'device.co')
            subprocess.run([os.path.join(LLVM_BIN, 'llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fb, path], check=True)
            subprocess.run([os.path.join(LLVM_BIN, 'clang-offload-bundler'), '--unbundle', '--type=o', '--targets=hipv4-amdgcn-amd-amdhsa--' + ARCH,
                            '--input=' + fb, '--output=' + co], check=True)
        return subprocess.run([os.path.join(LLVM_BIN, 'llvm-objdump'), '-d', '--symbolize-operands', '--no-show-raw-insn', co],
                              check=True, capture_output=True, text=True).stdout


def main(args):
    global ARCH
    paths = []
    for a in args:
        if a.startswith('--arch='):
            ARCH = a[len('--arch='):]
        else:
            paths.append(a)
    seen, failed = 0, 0
    for path in paths:
        for short, summary, bad, allowed in check_text(device_isa(path)):
            seen += 1
            mark = ''
            if bad and allowed:
                mark = '   (allowed: %s)' % allowed
            elif bad:
                failed += 1
                mark = '   <- ' + '; '.join(bad)
            print('  %-36s %s%s' % (short, summary, mark))
    if seen == 0:
        print('check_ring_waits: no ring loop found in', paths)
        return 2
    if failed:
        print('check_ring_waits: %d of %d ring loops do not keep their loads in flight (see above)' % (failed, seen))
        return 1
    print('check_ring_waits: %d ring loops, every group has its own wait' % seen)
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
