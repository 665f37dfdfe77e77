#!/usr/bin/env python
"""What surrounds the k loop of an MFMA kernel, from a gfx9 assembly listing: epilogue_order.py <file.s> [name filter ...].

A wave that has its SIMD to itself issues in order, so whatever the listing places in front of a memory operation is time
that operation starts later.  Per kernel with MFMAs this prints, following the listing's text (not its control flow: where
the epilogue has arms - full row tile / last row tile, C = / C += - the first arm in the text is what is measured),
  (a) epilogue   between the last MFMA and the first global store behind it: instructions, s_barrier, LDS operations
                 (ds_*, bpermutes included) and IEEE division sequences (v_div_fixup) - and the same counts, with
                 the global stores, between that first store and the end of the kernel,
  (b) prologue   global loads in front of the first operand-tile load (`early`; the first 16-byte global_load_dwordx4: the
                 staged units of er_gemm_core.h; `-` where a kernel stages with dword loads only.  The unaligned-operand
                 loop, which the text places in front of the aligned one, counts here with its own 16 dword loads and with
                 the epilogue operands requested on its path), the global loads between that load and the first ds_write
                 behind it (`behind`: the rest of the first two k-tiles and whatever else was requested there), and the
                 vmcnt of the last s_waitcnt in front of that ds_write (0: the first staging write waits for EVERY load
                 issued so far, epilogue operands included; n > 0: the n youngest loads stay in flight).
The listing comes from the build's own flags with -S (hipcc ... --cuda-device-only -S file.hip).  A report, not a test."""
import re
import sys

from store_waits import demangle, kernels

MFMA = re.compile(r'^\s+v_mfma_')
GSTORE = re.compile(r'^\s+global_store\w*\s')
GLOAD = re.compile(r'^\s+global_load\w*\s')
GLOAD4 = re.compile(r'^\s+global_load_dwordx4\s')
LDS = re.compile(r'^\s+ds_\w+\s')
DSWRITE = re.compile(r'^\s+ds_write\w*\s')
BARRIER = re.compile(r'^\s+s_barrier\b')
DIV = re.compile(r'^\s+v_div_fixup\w*\s')
VMCNT = re.compile(r'^\s+s_waitcnt\b.*\bvmcnt\((\d+)\)')


def span(body):
  return {'instr': len(body), 'barrier': sum(1 for l in body if BARRIER.match(l)), 'lds': sum(1 for l in body if LDS.match(l)),
          'div': sum(1 for l in body if DIV.match(l)), 'gstore': sum(1 for l in body if GSTORE.match(l)),
          'gload': sum(1 for l in body if GLOAD.match(l))}


def report(body):
  """-> (counts before the first store, counts behind it, first store, loads early, loads behind, vmcnt) or None"""
  mf = [i for i, l in enumerate(body) if MFMA.match(l)]
  if not mf:
    return None
  last = mf[-1]
  st = next((i for i in range(last + 1, len(body)) if GSTORE.match(body[i])), None)
  before = span(body[last + 1:st]) if st is not None else None
  after = span(body[st + 1:]) if st is not None else None
  first = body[st].split()[0] if st is not None else '-'
  op = next((i for i, l in enumerate(body) if GLOAD4.match(l)), None)
  early = behind = vm = None
  if op is not None:
    early = sum(1 for l in body[:op] if GLOAD.match(l))
    dw = next((i for i in range(op, len(body)) if DSWRITE.match(body[i])), None)
    if dw is not None:
      behind = sum(1 for l in body[op + 1:dw] if GLOAD.match(l))
      for l in body[op:dw]:
        m = VMCNT.match(l)
        if m:
          vm = int(m.group(1))
  return before, after, first, early, behind, vm


def main():
  with open(sys.argv[1]) as f:
    ks = kernels(f.read().split('\n'))
  filt = sys.argv[2:]
  names = demangle([k for k, _ in ks])
  fmt = '%5s %4s %4s %4s | %5s %4s %4s %4s %4s | %-22s | %5s %6s %5s  %s'
  print('(a) last MFMA -> first store    | first store -> end           |                        | (b) prologue')
  print(fmt % ('instr', 'bar', 'lds', 'div', 'instr', 'bar', 'lds', 'div', 'st', 'first store', 'early', 'behind', 'vmcnt', 'kernel'))
  for sym, body in sorted(ks, key=lambda kb: names[kb[0]]):
    name = re.sub(r'^void ', '', names[sym])
    if filt and not any(s in name for s in filt):
      continue
    r = report(body)
    if r is None or r[0] is None:
      continue
    b, a, first, early, behind, vm = r
    print(fmt % (b['instr'], b['barrier'], b['lds'], b['div'], a['instr'], a['barrier'], a['lds'], a['div'], a['gstore'], first,
                 '-' if early is None else early, '-' if behind is None else behind, '-' if vm is None else vm, name[:120]))


if __name__ == '__main__':
  main()
