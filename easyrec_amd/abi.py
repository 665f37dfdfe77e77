"""The C ABI of libeasyrec_hip.so as include/easyrec_hip.h states it, read from the header's text: the records
(`typedef struct { ... } er_name;` -> a ctypes.Structure), the constants (`enum { ER_.. }`, integer `#define ER_..`) and
the function signatures (bind_library).  Nothing of it is typed a second time in Python; what the parser cannot
represent is an error, never skipped.  The records and constants are read once, at import (RECORDS, CONSTANTS)."""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# EASYREC_AMD_LIB: another build of the same ABI (same-box A/B of a kernel change, tools/gpu_ab.sh)
LIB_PATH = os.environ.get('EASYREC_AMD_LIB') or os.path.join(_HERE, 'csrc', 'libeasyrec_hip.so')
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'easyrec_hip.h')

# C scalar types of the header -> ctypes; every pointer (and er_stream_t) is c_void_p, which also takes an int address,
# None, bytes, a ctypes array and byref()
_C_SCALARS = {'int': ctypes.c_int, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'uint32_t': ctypes.c_uint32,
              'uint64_t': ctypes.c_uint64, 'uint8_t': ctypes.c_uint8, 'float': ctypes.c_float, 'double': ctypes.c_double,
              'er_stream_t': ctypes.c_void_p}
_RENAMED = {'lambda': 'lam'}  # (a Python keyword)
_INT_LITERAL = re.compile(r'[-+]?(0[xX][0-9a-fA-F]+|0|[1-9]\d*)$')


def _ctype(decl, what, ret=False, records=()):
  decl = ' '.join(decl.replace('*', ' * ').split())
  if '*' in decl:
    return ctypes.c_char_p if ret and decl == 'const char *' else ctypes.c_void_p
  if decl in records:
    return records[decl]
  if decl not in _C_SCALARS:
    raise RuntimeError('easyrec_amd: %s: no ctypes type for %r' % (what, decl))
  return _C_SCALARS[decl]


def _int(text, what):
  if not _INT_LITERAL.match(text):
    raise RuntimeError('easyrec_amd: %s: %r is not an integer literal' % (what, text))
  return int(text, 0)


def _code(header):
  """The header's text without comments, and without comments and preprocessor lines."""
  with open(header) as f:
    text = re.sub(r'/\*.*?\*/', ' ', f.read(), flags=re.S)
  return text, re.sub(r'^\s*#.*$', '', text, flags=re.M)


def _record(name, body, records, header):
  """The ctypes.Structure of `typedef struct { body } name;`.  A declaration is `type declarator, declarator, ...;`, a
  declarator `[*..]field` or `[*..]field[n]`, the type a scalar of _C_SCALARS, anything pointed to, or an earlier record."""
  fields = []
  for decl in filter(None, (' '.join(d.split()) for d in body.split(';'))):
    what = '%s: %s field `%s`' % (header, name, decl)
    if re.search(r'[{}():]|^(union|struct|enum)\b', decl):  # nested aggregate, function pointer, bit-field
      raise RuntimeError('easyrec_amd: %s: no ctypes form for this declaration' % what)
    base = None
    for part in decl.split(','):
      m = re.match(r'(.*?)([\s*]*)\b(\w+)\s*(?:\[\s*(\w+)\s*\])?$', part.strip())
      if m is None or bool(m.group(1)) != (base is None):  # (the first declarator carries the type, the others none)
        raise RuntimeError('easyrec_amd: %s: cannot parse the declaration' % what)
      if base is None:
        base = m.group(1)
      ctype = _ctype(base + m.group(2), what, records=records)
      if m.group(4) is not None:
        ctype = ctype * _int(m.group(4), what + ' array length')
      fields.append((_RENAMED.get(m.group(3), m.group(3)), ctype))
  return type(name, (ctypes.Structure,), {'_fields_': fields, '__doc__': '%s (include/easyrec_hip.h)' % name})


def parse_header(header=HEADER_PATH):
  """(records, constants) of the header: {er_name: its ctypes.Structure subclass} for every `typedef struct` with a body
  and {ER_NAME: int} for every enum name and `#define ER_NAME`.  A struct or union defined in any other form, a field or
  a value with no ctypes / int form is an error."""
  text, code = _code(header)
  constants = {}
  for name, value in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(ER_\w+)(.*)$', text, flags=re.M):
    constants[name] = _int(value.strip(), '%s: #define %s' % (header, name))
  for body in re.findall(r'\benum\s*\w*\s*\{([^{}]*)\}', code):
    value = -1
    for entry in filter(None, (e.strip() for e in body.split(','))):
      name, eq, literal = (s.strip() for s in entry.partition('='))
      value = _int(literal, '%s: enum %s' % (header, name)) if eq else value + 1
      constants[name] = value
  records, rest, last = {}, '', 0  # rest: the code outside the bodies that became records
  for m in re.finditer(r'\btypedef\s+struct\s*\w*\s*\{', code):
    end, depth = m.end(), 1
    while depth and end < len(code):
      depth += {'{': 1, '}': -1}.get(code[end], 0)
      end += 1
    name = re.match(r'\s*(\w+)\s*;', code[end:])
    if depth or name is None:
      raise RuntimeError('easyrec_amd: %s: cannot parse the struct at `%s`' % (header, m.group(0)))
    records[name.group(1)] = _record(name.group(1), code[m.end():end - 1], records, header)
    rest, last = rest + code[last:m.start()], end
  n_bodies = len(re.findall(r'\btypedef\s+struct\b[^;{]*\{', code))
  if len(records) != n_bodies:
    raise RuntimeError('easyrec_amd: %s: %d records built from %d `typedef struct` bodies' % (header, len(records), n_bodies))
  stray = re.search(r'\b(struct|union)\b[^;{()]*\{', rest + code[last:])
  if stray:
    raise RuntimeError('easyrec_amd: %s: `%s` defines a struct or union that is no `typedef struct { ... } er_name;`' %
                       (header, ' '.join(stray.group(0).split())))
  return records, constants


RECORDS, CONSTANTS = parse_header()  # (the one class there is for each C struct; every ER_ constant)


def load_library(path=LIB_PATH, header=HEADER_PATH):
  """Open libeasyrec_hip.so and bind it (bind_library)."""
  if not os.path.exists(path):
    raise RuntimeError(
        'easyrec_amd: %s not found. Build it with `python -c "import __graft_entry__ as g; '
        'g.build()"` or `make -C easyrec_amd/csrc`; there is no CPU fallback.' % path)
  return bind_library(ctypes.CDLL(path), header)


def bind_library(lib, header=HEADER_PATH):
  """Give every function the header declares argtypes / restype on `lib` (a ctypes.CDLL of libeasyrec_hip.so), so that
  ctypes converts (and type-checks) each argument as the header says: plain Python ints / floats / bools for scalars, an
  address, None, bytes, a ctypes array or byref() for pointers.  Returns lib."""
  for ret, name, params in re.findall(r'([\w\s*]+?)\b(er_\w+)\s*\(([^()]*)\)\s*;', _code(header)[1]):
    params = ' '.join(params.split())
    decls = [] if params in ('', 'void') else [re.sub(r'\w+$', '', p) for p in params.split(',')]
    if not hasattr(lib, name):
      raise RuntimeError('easyrec_amd: %s declares %s, %s does not export it' % (header, name, lib._name))
    fn = getattr(lib, name)
    fn.restype = _ctype(ret, '%s: %s return type' % (header, name), ret=True)
    fn.argtypes = [_ctype(d, '%s: %s argument %d' % (header, name, i + 1)) for i, d in enumerate(decls)]
  return lib
