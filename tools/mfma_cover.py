#!/usr/bin/env python
"""MFMA cover of the waits in a kernel's innermost loop, from a gfx9 assembly listing: mfma_cover.py <file.s> [name filter ...].

A wave issues in order, and an MFMA that accumulates into the registers of the one before it is issued when that one
leaves the pipe.  What a memory operation has for cover is therefore the number of MFMAs that stand between it and the
`s_waitcnt` that waits for it: an LDS read issued behind a group of four dependent MFMAs runs under the last of them only.
Per kernel this walks the innermost loop with the most MFMAs (the loop whose header the listing marks `Inner Loop
Header`, its blocks in the listing's order, starting at the header; walked twice so that the operations in flight at the
top are those of the previous iteration) and prints, for every
  s_waitcnt lgkmcnt(n) / vmcnt(n)   the youngest operation it waits for (the LDS and the vector memory return in order:
                                    all but the n youngest in flight) and the MFMAs issued between that operation and
                                    the wait,
  s_barrier                         the MFMAs issued since the youngest LDS write and the youngest LDS read before it,
and, at the end, the loop's MFMA count and the smallest cover per kind.  Operations are followed along the listing's
order: where the loop has branches, a wait's operation may lie in a block that does not always run in front of it (the
block labels are printed).  The listing comes from the build's own flags with -S (hipcc ... --cuda-device-only -S
file.hip).  A report, not a test."""
import re
import sys

from store_waits import demangle, kernels

MFMA = re.compile(r'^\s+v_mfma_')
LGKM = re.compile(r'^\s+(ds_\w+|s_load_\w+|s_buffer_load_\w+)\s')
VMEM = re.compile(r'^\s+((global|buffer|flat|scratch)_(load|store|atomic)\w*)\s')
LABEL = re.compile(r'^(\.LBB\d+_\d+):')
HEADER = re.compile(r'^(\.LBB\d+_\d+):.*=>This Inner Loop Header')
IN_LOOP = re.compile(r'in Loop: Header=(BB\d+_\d+)')


def kernel_lines(lines):
  """-> {symbol: [every line of the kernel's text, labels and comments included]}"""
  names = {k for k, _ in kernels(lines)}
  out, cur = {}, None
  for ln in lines:
    m = re.match(r'^([A-Za-z_.$][\w.$]*):', ln)
    if m and m.group(1) in names:
      cur = m.group(1)
      out[cur] = []
      continue
    if cur and ln.startswith('.Lfunc_end'):
      cur = None
    if cur:
      out[cur].append(ln)
  return out


def inner_loops(body):
  """-> [[lines]] of the kernel's innermost loops, each rotated to start at its header"""
  blocks, cur = [], None  # (label, header-of-loop or None, is-header, lines)
  for ln in body:
    m = LABEL.match(ln)
    if m:
      h = IN_LOOP.search(ln)
      cur = [m.group(1), ('.L' + h.group(1)) if h else None, bool(HEADER.match(ln)), [ln]]
      blocks.append(cur)
    elif cur is not None:
      cur[3].append(ln)
  loops = []
  for lab, _, is_head, _ in blocks:
    if not is_head:
      continue
    member = [b for b in blocks if b[0] == lab or b[1] == lab]
    at = next(i for i, b in enumerate(member) if b[0] == lab)
    member = member[at:] + member[:at]
    loops.append([ln for b in member for ln in b[3]])
  return loops


def count_of(text, what):
  m = re.search(what + r'\((\d+)\)', text)
  return int(m.group(1)) if m else None


def walk(loop):
  """-> (report lines, MFMAs per trip, {kind: smallest cover})"""
  rep, worst = [], {}
  lgkm, vm = [], []  # in flight: (mnemonic, MFMAs issued before it, line number in the loop)
  lds = []  # every LDS operation issued so far, in order
  mfmas = 0
  for trip in (0, 1):
    show = trip == 1
    for n, ln in enumerate(loop):
      text = ln.split(';')[0].rstrip()
      if LABEL.match(ln):
        if show:
          rep.append('%s' % ln.split()[0])
        continue
      if MFMA.match(text):
        mfmas += 1
        continue
      m = LGKM.match(text)
      if m:
        lgkm.append((m.group(1), mfmas, n))
        if m.group(1).startswith('ds_'):
          lds.append(lgkm[-1])
        continue
      m = VMEM.match(text)
      if m:
        vm.append((m.group(1), mfmas, n))
        continue
      if re.match(r'^\s+s_waitcnt\b', text):
        for what, q in (('lgkmcnt', lgkm), ('vmcnt', vm)):
          left = count_of(text, what)
          if left is None or len(q) <= left:
            continue
          op, at, line = q[len(q) - left - 1]
          del q[:len(q) - left]
          if show:
            rep.append('  %4d  s_waitcnt %-12s waits for %-20s (loop line %4d): %2d MFMAs of cover' %
                       (n, '%s(%d)' % (what, left), op, line, mfmas - at))
            kind = what + (' (ds_read)' if op.startswith('ds_read') else ' (ds_write)' if op.startswith('ds_write') else '')
            worst[kind] = min(worst.get(kind, 1 << 30), mfmas - at)
        continue
      if re.match(r'^\s+s_barrier\b', text) and show:
        part = []
        for kind in ('ds_write', 'ds_read'):
          last = [x for x in lds if x[0].startswith(kind)]
          if last:
            part.append('%d MFMAs since the youngest %s' % (mfmas - last[-1][1], kind))
            worst['s_barrier (%s)' % kind] = min(worst.get('s_barrier (%s)' % kind, 1 << 30), mfmas - last[-1][1])
        rep.append('  %4d  s_barrier: %s' % (n, ', '.join(part)))
  return rep, mfmas // 2, worst


def main():
  with open(sys.argv[1]) as f:
    lines = f.read().split('\n')
  filt = sys.argv[2:]
  bodies = kernel_lines(lines)
  names = demangle(list(bodies))
  for sym in sorted(bodies, key=lambda s: names[s]):
    name = re.sub(r'^void ', '', names[sym])
    if filt and not any(s in name for s in filt):
      continue
    loops = inner_loops(bodies[sym])
    loops = [l for l in loops if any(MFMA.match(ln) for ln in l)]
    if not loops:
      continue
    loop = max(loops, key=lambda l: sum(1 for ln in l if MFMA.match(ln)))
    rep, per_trip, worst = walk(loop)
    print('%s' % name[:150])
    print('  innermost loop: %d lines, %d MFMAs per trip' % (len(loop), per_trip))
    print('\n'.join(rep))
    print('  smallest cover: ' + ', '.join('%s %d' % kv for kv in sorted(worst.items())))
    print()


if __name__ == '__main__':
  main()
