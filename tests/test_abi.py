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
  """What the header's readers cannot represent stops them: a signature (load_library), a record field or a constant
  (abi.parse_header) is never skipped."""
  from easyrec_amd import abi, kernels

  def bind(header):
    monkeypatch.setattr(kernels, 'HEADER_PATH', header)
    kernels.load_library(built_lib)

  for read, proto, what in (
      (bind, 'int er_abi_version(long x);', 'no ctypes type'), (bind, 'int er_not_exported(void);', 'does not export'),
      (abi.parse_header, 'typedef struct { int32_t n; long x; } er_bad;', "er_bad field `long x`: no ctypes type for 'long'"),
      (abi.parse_header, 'typedef struct er_bad { int32_t n; int32_t flag : 1; } er_bad;', 'er_bad field `int32_t flag : 1`'),
      (abi.parse_header, 'typedef struct { int32_t n; union { float f; int32_t i; } u; } er_bad;', 'er_bad field `union'),
      (abi.parse_header, 'typedef struct { int32_t n; struct { float f; } s; } er_bad;', 'er_bad field `struct'),
      (abi.parse_header, 'typedef struct { int32_t n; int (*fn)(int32_t); } er_bad;', r'er_bad field `int \(\*fn\)\(int32_t\)`'),
      (abi.parse_header, 'typedef struct __attribute__((packed)) { int32_t n; } er_bad;', '0 records built from 1'),
      (abi.parse_header, 'struct er_bad { int32_t n; };', '`struct er_bad {` defines a struct or union'),
      (abi.parse_header, 'typedef union { float f; int32_t i; } er_bad;', '`union {` defines a struct or union'),
      (abi.parse_header, '#define ER_X (1 << 2)', "#define ER_X: '\\(1 << 2\\)' is not an integer literal"),
      (abi.parse_header, 'enum { ER_Y = ER_X + 1 };', 'enum ER_Y')):
    header = tmp_path / 'easyrec_hip.h'
    header.write_text('/* int er_commented_out(void); */\n' + proto + '\n')
    with pytest.raises(RuntimeError, match=what):
      read(str(header))
  header.write_text('typedef struct er_opaque er_opaque;\ntypedef struct { int32_t a, b; float* p; } er_ok;\nenum { ER_A, ER_B };\n')
  records, constants = abi.parse_header(str(header))  # (and what it can represent, it reads)
  assert [(n, t.__name__) for n, t in records['er_ok']._fields_] == [('a', 'c_int'), ('b', 'c_int'), ('p', 'c_void_p')]
  assert list(records) == ['er_ok'] and constants == {'ER_A': 0, 'ER_B': 1}


def test_a_failed_call_is_reported_under_the_name_of_the_function_called(built_lib, tmp_path):
  """HipBackend.ck.er_NAME(...) raises for a non-zero return code, naming er_NAME itself and quoting er_last_error().
  er_load_dense_embed fails on the host (no such checkpoint folder) before anything touches a device."""
  from easyrec_amd import kernels
  be = kernels.HipBackend.__new__(kernels.HipBackend)  # (a host-only backend)
  be.lib = ctypes.CDLL(built_lib)
  with pytest.raises(RuntimeError) as err:
    be.load_dense_embed(str(tmp_path / 'nope'), 'var', 0, 1, 4, 8)
  reason = be.lib.er_last_error().decode()
  assert 'cannot list' in reason and str(tmp_path) in reason
  rc = be.lib.er_load_dense_embed(str(tmp_path / 'nope').encode(), b'var', 0, 1, 4, 8, None, None)
  assert rc != 0 and str(err.value) == 'er_load_dense_embed failed (rc=%d): %s' % (rc, reason)
  first = be.ck.er_load_dense_embed
  assert be.ck.er_load_dense_embed is first  # (built once per name)
  be.lib = ctypes.CDLL(built_lib)  # another library handed over: the checked calls are built again, for that library
  assert be.ck.er_load_dense_embed is not first
  with pytest.raises(RuntimeError, match=r'^er_save_dense_embed failed \(rc=\d+\): er_save_dense_embed: '):
    be.ck.er_save_dense_embed(None, None, 0, 1, None, 0, 0)
  with pytest.raises(AttributeError):
    be.ck.er_no_such_function


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


def test_constants_read_from_the_header_have_the_values_the_library_was_built_with():
  """kernels.py takes every constant from include/easyrec_hip.h; these are the values, stated by hand, that the kernels
  switch on."""
  from easyrec_amd import kernels as k
  assert (k.COMBINER_SUM, k.COMBINER_MEAN, k.COMBINER_SQRTN) == (0, 1, 2)
  assert k.COMBINERS == {'sum': 0, 'mean': 1, 'sqrtn': 2}
  assert (k.OPT_SGD, k.OPT_ADAM, k.OPT_LAZY_ADAM, k.OPT_ADAGRAD) == (0, 1, 2, 3)
  assert (k.ACT_NONE, k.ACT_RELU) == (0, 1)
  assert (k.BN_NONE, k.BN_BATCH, k.BN_FROZEN) == (0, 1, 2)
  assert (k.GEMM_NN, k.GEMM_NT, k.GEMM_TN) == (0, 1, 2)
  assert (k.EPI_PLAIN, k.EPI_STATS, k.EPI_BN_BWD, k.EPI_CROSS_FWD, k.EPI_CROSS_BWD) == (0, 1, 2, 3, 4)
  assert (k.GRAD_TERM_ROWSUM, k.GRAD_TERM_FM) == (0, 1)
  assert (k.HYPER_LR, k.HYPER_LR_T, k.HYPER_BETA1, k.HYPER_BETA2, k.HYPER_OMB1, k.HYPER_OMB2, k.HYPER_EPS,
          k.HYPER_GSCALE) == tuple(range(8))
  assert k.HYPER_CLIP == 8
  assert (k.FRONT_SKIP_ONE_ROW, k.FRONT_DEFER_CATCH_UP, k.ABI_VERSION) == (1, 2, 1)


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


RENAMED = {'lam': 'lambda'}  # (a Python keyword on the C side)


def test_every_ctypes_mirror_has_the_size_and_field_offsets_of_its_c_struct(tmp_path):
  """The host side hands the library arrays of records: a ctypes record that differs from include/easyrec_hip.h (a field
  dropped, reordered or of another width) would corrupt every call silently.  abi.py lays each class out from the field
  list it parsed; here the header is compiled as C (gcc) into a probe that prints sizeof and every field's offsetof and
  size: every record the header defines must agree, field by field - padding and reserved fields included."""
  import shutil
  import subprocess
  from easyrec_amd import abi, kernels
  if shutil.which('gcc') is None:
    import pytest
    pytest.skip('no gcc')
  assert len(abi.RECORDS) == 16 and abi.RECORDS['er_opt_hyper'] is kernels.OptHyper
  assert abi.RECORDS['er_grad_group'].terms.size == 4 * ctypes.sizeof(kernels.GradTerm)
  assert dict(abi.RECORDS['er_grad_group']._fields_)['terms']._type_ is kernels.GradTerm  # (ONE class per C struct)
  assert {name for name, v in vars(kernels).items() if isinstance(v, type) and issubclass(v, ctypes.Structure)} == {
      'GemmEpilogue', 'LookupDesc', 'KvJob', 'KvRouteJob', 'CastDesc', 'GemmProblem', 'BnLayer', 'CeHead', 'TailJob',
      'LossTailJob', 'DenseOptJob', 'GradTerm', 'GradGroup', 'DenseApplyDesc', 'ColsumJob', 'OptHyper'}
  lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "easyrec_hip.h"', 'int main(void) {']
  for c_name, cls in abi.RECORDS.items():
    lines.append('  printf("%s size %%zu 0\\n", sizeof(%s));' % (c_name, c_name))
    for fname, _ in cls._fields_:
      lines.append('  printf("%s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' %
                   (c_name, fname, c_name, RENAMED.get(fname, fname), c_name, RENAMED.get(fname, fname)))
  lines += ['  return 0;', '}']
  src = tmp_path / 'probe.c'
  src.write_text('\n'.join(lines))
  exe = tmp_path / 'probe'
  subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
  out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
  got = {}
  for ln in out.splitlines():
    c_name, key, val, size = ln.split()
    got[(c_name, key)] = (int(val), int(size))
  n_fields = 0
  for c_name, cls in abi.RECORDS.items():
    assert ctypes.sizeof(cls) == got[(c_name, 'size')][0], (c_name, ctypes.sizeof(cls), got[(c_name, 'size')])
    for fname, _ in cls._fields_:
      n_fields += 1
      assert (getattr(cls, fname).offset, getattr(cls, fname).size) == got[(c_name, fname)], (c_name, fname)
  assert n_fields == len(got) - len(abi.RECORDS) and n_fields > 200
