#!/usr/bin/env python
"""Stores and the waits between them, per kernel, from a gfx9 assembly listing: store_waits.py <file.s> [name filter ...].

On gfx9-family hardware a vector store counts in vmcnt like a load, so an `s_waitcnt vmcnt(0)` that follows a store waits
for that store's acknowledgement.  An epilogue whose stores sit in per-element branches gets such a wait in front of every
store after the first: the stores of a lane then leave one round trip apart.  Per kernel this prints
  stores   global_store* / buffer_store* instructions
  between  s_waitcnt with vmcnt(0) that have a store before them and a store after them in the kernel's text
  chained  of those, the ones whose next store follows within WINDOW instructions - the waits that serialise a run of stores
The listing comes from the build's own flags with -S (hipcc ... --cuda-device-only -S file.hip).  A report, not a test."""
import re
import subprocess
import sys

WINDOW = 12
STORE = re.compile(r'^\s+(global_store|buffer_store)\w*\s')
WAIT0 = re.compile(r'^\s+s_waitcnt\b.*\bvmcnt\(0\)')
INSTR = re.compile(r'^\s+[a-z]\w*(\s|$)')


def kernels(lines):
  """-> [(symbol, [instruction lines])] of the .amdhsa kernels in the listing"""
  names = set(re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', '\n'.join(lines), re.M))
  out, cur, body = [], None, []
  for ln in lines:
    m = re.match(r'^([A-Za-z_.$][\w.$]*):', ln)
    if m and m.group(1) in names:
      cur, body = m.group(1), []
      continue
    if cur and ln.startswith('.Lfunc_end'):
      out.append((cur, body))
      cur = None
      continue
    if cur and INSTR.match(ln) and not ln.lstrip().startswith('.'):
      body.append(ln)
  return out


def demangle(syms):
  try:
    res = subprocess.run(['c++filt'], input='\n'.join(syms), capture_output=True, text=True, check=True).stdout.split('\n')
    return dict(zip(syms, res))
  except (OSError, subprocess.CalledProcessError):
    return {s: s for s in syms}


def count(body):
  st = [i for i, ln in enumerate(body) if STORE.match(ln)]
  if not st:
    return 0, 0, 0
  between = chained = 0
  for i, ln in enumerate(body):
    if WAIT0.match(ln) and st[0] < i < st[-1]:
      between += 1
      nxt = next(s for s in st if s > i)
      if nxt - i <= WINDOW:
        chained += 1
  return len(st), between, chained


def main():
  with open(sys.argv[1]) as f:
    ks = kernels(f.read().split('\n'))
  filt = sys.argv[2:]
  names = demangle([k for k, _ in ks])
  print('%-7s %-8s %-8s kernel' % ('stores', 'between', 'chained'))
  for sym, body in sorted(ks, key=lambda kb: names[kb[0]]):
    name = re.sub(r'^void ', '', names[sym])
    if filt and not any(s in name for s in filt):
      continue
    print('%-7d %-8d %-8d %s' % (count(body) + (name[:150],)))


if __name__ == '__main__':
  main()
