"""The C-ABI library loads on a machine without a GPU and exports every symbol declared in
include/easyrec_hip.h (no compute calls here)."""
import ast
import ctypes
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
  text = open(os.path.join(ROOT, 'include', 'easyrec_hip.h')).read()
  return re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def declared_symbols():
  return sorted(set(re.findall(r'\b(er_[a-z0-9_]+)\s*\(', _header())))


def declared_param_counts():
  """name -> the number of parameters of its prototype in include/easyrec_hip.h"""
  protos = re.findall(r'\b(er_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', _header())
  return {name: 0 if params.strip() in ('', 'void') else params.count(',') + 1 for name, params in protos}


def test_header_declares_the_hot_path():
  syms = declared_symbols()
  for must in ('er_hash_bucket_fast', 'er_emb_fwd', 'er_emb_bwd_update', 'er_fm_fwd', 'er_cross_v1_fwd',
               'er_cross_v2_epilogue_fwd', 'er_din_pool_fwd', 'er_bn_act_fwd', 'er_sigmoid_ce_fwd_bwd',
               'er_mmoe_mix_fwd', 'er_dense_opt_step', 'er_adam_decay_sweep'):
    assert must in syms


def test_library_exports_every_declared_symbol(built_lib):
  lib = ctypes.CDLL(built_lib)
  missing = [s for s in declared_symbols() if not hasattr(lib, s)]
  assert not missing, 'declared in include/easyrec_hip.h but not exported: %s' % missing
  assert lib.er_abi_version() == 1


def test_every_declared_function_is_bound_to_its_header_signature(built_lib):
  """kernels.load_library gives every function of the header argtypes and restype: ctypes then converts each argument
  to the declared width and rejects what does not fit (a ctypes scalar of another width, a float for a pointer)."""
  from easyrec_amd import kernels
  c = ctypes
  lib = kernels.load_library(built_lib)
  counts = declared_param_counts()
  assert sorted(counts) == declared_symbols()
  bound = sorted(name for name, fn in vars(lib).items() if name.startswith('er_') and fn.argtypes is not None)
  assert bound == declared_symbols()
  for name, n in counts.items():
    assert len(getattr(lib, name).argtypes) == n, name
  i32, vp = c.c_int32, c.c_void_p
  assert lib.er_gemm_f32.argtypes == [c.c_int, i32, i32, i32, vp, i32, vp, i32, vp, i32, vp, c.c_int, vp, vp]
  assert lib.er_gemm_f32.restype is c.c_int
  assert lib.er_last_error.argtypes == [] and lib.er_last_error.restype is c.c_char_p
  assert lib.er_emb_group_num_entries.argtypes == [vp] and lib.er_emb_group_num_entries.restype is c.c_int64
  assert lib.er_crc32c.argtypes == [c.c_uint32, vp, c.c_int64] and lib.er_crc32c.restype is c.c_uint32
  assert lib.er_bst_grid.argtypes == [c.c_int64] and lib.er_bst_grid.restype is c.c_int32
  assert lib.er_reduce_sum.argtypes[2] is c.c_float and lib.er_decode_csv_host.argtypes[2] is c.c_uint8
  assert lib.er_debug_stamps.argtypes == [vp]  # (unsigned long long*)
  assert lib.er_crc32c(0, b'123456789', 9) == 0xE3069283  # (CRC-32C check value; bytes for a const void*)
  be = kernels.HipBackend.__new__(kernels.HipBackend)  # (a host-only backend: no device touched)
  be.lib = ctypes.CDLL(built_lib)                       # a library opened elsewhere is bound when it is handed over
  assert be.lib.er_crc32c.argtypes == [c.c_uint32, vp, c.c_int64] and be.lib.er_last_error.restype is c.c_char_p
  bst_grid = lib.er_bst_grid
  with pytest.raises(ctypes.ArgumentError):
    bst_grid(ctypes.c_int32(4096))  # an explicit cast of the wrong width


def test_binder_refuses_unknown_types_and_missing_exports(built_lib, monkeypatch, tmp_path):
  from easyrec_amd import kernels
  for proto, what in (('int er_abi_version(long x);', 'no ctypes type'), ('int er_not_exported(void);', 'does not export')):
    header = tmp_path / 'easyrec_hip.h'
    header.write_text('/* int er_commented_out(void); */\n' + proto + '\n')
    monkeypatch.setattr(kernels, 'HEADER_PATH', str(header))
    with pytest.raises(RuntimeError, match=what):
      kernels.load_library(built_lib)


def _library_calls():
  """(file, line, NAME, call node) of every call <...>.er_NAME(...) in the package, the tools, the tests and the entry
  points"""
  paths = [os.path.join(ROOT, '__graft_entry__.py')] + sorted(glob.glob(os.path.join(ROOT, 'tools', '*.py')))
  for top in ('easyrec_amd', 'tests'):
    for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
      paths += [os.path.join(dirpath, f) for f in sorted(files) if f.endswith('.py')]
  for path in paths:
    tree = ast.parse(open(path).read(), path)
    for node in ast.walk(tree):
      if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr.startswith('er_'):
        yield os.path.relpath(path, ROOT), node.lineno, node.func.attr, node


def test_every_library_call_site_matches_the_header(built_lib):
  """argtypes alone does not catch a call with one argument too many: CPython's ctypes rejects too FEW arguments to a
  CDLL (cdecl) function with TypeError, but passes surplus ones on without a word (checked below on a host-side entry
  point).  So every call <...>.er_NAME(...) must name a declared function and, unless it unpacks *args, pass exactly the
  declared number of positional arguments."""
  from easyrec_amd import kernels
  lib = kernels.load_library(built_lib)
  row_tiles = lib.er_gemm_row_tiles
  with pytest.raises(TypeError):
    row_tiles()
  assert row_tiles(1000, 12345) == row_tiles(1000)  # (the surplus argument is dropped)
  counts = declared_param_counts()
  bad, n_calls = [], 0
  for path, line, name, node in _library_calls():
    n_calls += 1
    if name not in counts:
      bad.append('%s:%d: %s is not declared in include/easyrec_hip.h' % (path, line, name))
    elif node.keywords or (len(node.args) != counts[name] and not any(isinstance(a, ast.Starred) for a in node.args)):
      bad.append('%s:%d: %s gets %d arguments%s, the header declares %d' %
                 (path, line, name, len(node.args), ' and keywords' if node.keywords else '', counts[name]))
  assert n_calls > 150, n_calls  # (the scan sees the call sites)
  assert not bad, bad


def test_struct_layout_matches_header(built_lib):
  from easyrec_amd import kernels
  # er_lookup_desc: 5 pointers + 2 int64 + 7 int32 = 40 + 16 + 28 = 84, padded to the 8-byte alignment: 88 bytes
  assert ctypes.sizeof(kernels.LookupDesc) == 88
  assert kernels.HYPER_FLOATS == 16


def test_product_does_not_import_the_oracle():
  """easyrec_amd/ must never import oracle/ (the product path has no CPU fallback)."""
  bad = []
  for dirpath, _, files in os.walk(os.path.join(ROOT, 'easyrec_amd')):
    for f in files:
      if f.endswith('.py'):
        src = open(os.path.join(dirpath, f)).read()
        if re.search(r'^\s*(from|import)\s+oracle\b', src, flags=re.M):
          bad.append(os.path.join(dirpath, f))
  assert not bad, bad


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
  import pytest
  from easyrec_amd import kernels
  monkeypatch.setattr(kernels, 'LIB_PATH', str(tmp_path / 'nope.so'))
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    kernels.HipBackend()


MIRRORS = {  # ctypes class in easyrec_amd/kernels.py -> the C struct it mirrors
    'GemmEpilogue': 'er_gemm_epilogue', 'LookupDesc': 'er_lookup_desc', 'KvJob': 'er_kv_job', 'KvRouteJob': 'er_kv_route_job', 'CastDesc': 'er_cast_desc',
    'GemmProblem': 'er_gemm_problem', 'BnLayer': 'er_bn_layer', 'CeHead': 'er_ce_head', 'TailJob': 'er_tail_job',
    'LossTailJob': 'er_loss_tail_job', 'DenseOptJob': 'er_dense_opt_job', 'GradTerm': 'er_grad_term',
    'GradGroup': 'er_grad_group', 'DenseApplyDesc': 'er_dense_apply_desc', 'ColsumJob': 'er_colsum_job',
}


RENAMED = {('GradGroup', 'lam'): 'lambda'}  # (a Python keyword on the C side)


def test_every_ctypes_mirror_has_the_size_and_field_offsets_of_its_c_struct(tmp_path):
  """The host side hands the library arrays of records: a ctypes mirror that drifts from include/easyrec_hip.h (a field
  dropped on one side only) would corrupt every call silently.  The header is compiled as C (gcc) into a probe that prints
  sizeof and every field's offsetof; the mirrors must agree field by field, in order."""
  import shutil
  import subprocess
  from easyrec_amd import kernels
  if shutil.which('gcc') is None:
    import pytest
    pytest.skip('no gcc')
  lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "easyrec_hip.h"', 'int main(void) {']
  for cls_name, c_name in MIRRORS.items():
    cls = getattr(kernels, cls_name)
    lines.append('  printf("%s size %%zu\\n", sizeof(%s));' % (c_name, c_name))
    for field in cls._fields_:
      fname = field[0]
      if fname.endswith('_') and fname.startswith('pad'):
        continue
      lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (c_name, fname, c_name, RENAMED.get((cls_name, fname), fname)))
  lines += ['  return 0;', '}']
  src = tmp_path / 'probe.c'
  src.write_text('\n'.join(lines))
  exe = tmp_path / 'probe'
  subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
  out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
  got = {}
  for ln in out.splitlines():
    c_name, key, val = ln.split()
    got[(c_name, key)] = int(val)
  for cls_name, c_name in MIRRORS.items():
    cls = getattr(kernels, cls_name)
    assert ctypes.sizeof(cls) == got[(c_name, 'size')], (cls_name, ctypes.sizeof(cls), got[(c_name, 'size')])
    for field in cls._fields_:
      fname = field[0]
      if (c_name, fname) in got:
        assert getattr(cls, fname).offset == got[(c_name, fname)], (cls_name, fname)
