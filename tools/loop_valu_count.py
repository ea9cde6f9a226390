#!/usr/bin/env python3
"""Vector instructions per step in the step loops of rollout_swar_kernel, from build/asm/soccer_rollout.s
(make -C gym_soccer_littman94_amd/csrc asm).

A kernel holds two step loops (the depth-2 loops of the assembly), the GENERAL = true one and the steady-state
(GENERAL = false) one, in the order the compiler chose.  A loop's basic blocks are split into the once-per-eight-ticks blocks — those that park or
fetch actions (ds_write / global_load) or run Philox rounds (v_mad_u64_u32; with slip they run every tick and count) —
the block of the per-lane return sums (v_pk_add_u16), which a run of steps never asks for, and the per-step blocks; the
count of a step is the number of v_* lines in the per-step blocks (the three moves of the odd-tick block count in full).
The smaller of the two loops is the steady state.

Usage: tools/loop_valu_count.py [--asm FILE] [--blocks] TEMPLATE_ARGS ...     e.g.  0,0,1,false  0,2,1,false,false"""
import argparse, collections, re, sys

ap = argparse.ArgumentParser()
ap.add_argument('--asm', default='build/asm/soccer_rollout.s')
ap.add_argument('--blocks', action='store_true', help='list every basic block of the loops')
ap.add_argument('--mix', action='store_true', help='the per-step blocks by opcode')
ap.add_argument('shapes', nargs='*', default=['0,0,1,false'])
a = ap.parse_args()


def mangled(shape):
    out = ''
    for x in shape.split(','):
        x = x.strip()
        out += 'Lb%dE' % (x == 'true') if x in ('true', 'false') else 'Li%sE' % x
    return '_ZN6soccer19rollout_swar_kernelI' + out + 'EEvNS_11RolloutSwarENS_9RolloutIOE'


lines = open(a.asm).read().split('\n')
for shape in a.shapes:
    name = mangled(shape)
    try:
        start = lines.index(name + ':') if name + ':' in lines else next(i for i, l in enumerate(lines) if l.startswith(name + ':'))
    except StopIteration:
        print('%s: not in %s' % (shape, a.asm)); continue
    end = next(i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end'))
    # depth-2 loops: from the header label to the backward branch to it
    loops = []
    for i in range(start, end):
        m = re.match(r'^(\.LBB\d+_\d+):.*Parent Loop', lines[i])
        if m and 'Loop Header: Depth=2' in lines[i + 1]:
            # the loop's last block is the last one whose comment names this header; it runs to the next label
            last = max(j for j in range(i, end) if 'Header=%s ' % m.group(1)[2:] in lines[j])
            back = next(j for j in range(last + 1, end + 1) if re.match(r'^(\.LBB\d+_\d+:|; %bb\.\d+:|\.Lfunc_end)', lines[j])) - 1
            loops.append((m.group(1), i, back))
    for k, (label, lo, hi) in enumerate(loops):
        blocks, cur = [], [label, []]
        for l in lines[lo + 1:hi + 1]:
            m = re.match(r'^(\.LBB\d+_\d+):', l) or re.match(r'^; (%bb\.\d+):', l)
            if m:
                blocks.append(cur); cur = [m.group(1), []]
            else:
                t = l.strip()
                if t and not t.startswith(('.', ';')):
                    cur[1].append(t.split()[0])
        blocks.append(cur)
        step = rare = acc = 0
        mix = collections.Counter()
        SLIP = shape.split(',')[1].strip() != '0'
        for lab, ins in blocks:
            v = sum(1 for x in ins if x.startswith('v_'))
            is_rare = any(x.startswith(('ds_write', 'global_load')) or x in ('v_mul_hi_u32', 'v_mad_u64_u32') for x in ins)
            is_acc = 'v_pk_add_u16' in ins                 # per-lane returns / episode counts: not asked for by a run of steps
            if SLIP: is_rare = False                       # slip: one Philox block per tick, part of the step
            if is_acc: acc += v
            elif is_rare: rare += v
            else:
                step += v; mix.update(x for x in ins if x.startswith('v_'))
            if a.blocks:
                print('    %-12s v %3d  all %3d  %s' % (lab, v, len(ins), 'per-lane sums' if is_acc else 'per eight ticks' if is_rare else 'per step'))
        readlane = sum(1 for _, ins in blocks for x in ins if x == 'v_readlane_b32')
        print('<%s> loop %d of %d (%s): per step %d v_*, per eight ticks %d v_*, per-lane sums %d v_*, v_readlane_b32 %d'
              % (shape, k + 1, len(loops), label, step, rare, acc, readlane))
        if a.mix:
            print('    ' + ', '.join('%s %d' % kv for kv in sorted(mix.items())))
