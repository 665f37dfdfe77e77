"""ctypes binding of libeasyrec_hip.so (include/easyrec_hip.h) at tensor level.

The reference issues this work as TensorFlow ops from Python (file:line cited per entry point in
include/easyrec_hip.h); here the same Python call sites call hand-written gfx950 kernels.

`hip()` returns the singleton `HipBackend`.  It fails loudly (RuntimeError) when the shared
library has not been built or no MI355X is visible - there is no CPU fallback in this package.
"""
import ctypes
import threading
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from easyrec_amd import abi
from easyrec_amd.abi import HEADER_PATH, LIB_PATH


def load_library(path=LIB_PATH):
  """Open libeasyrec_hip.so and bind it to this module's HEADER_PATH (abi.load_library)."""
  return abi.load_library(path, HEADER_PATH)


def bind_library(lib):
  """abi.bind_library with this module's HEADER_PATH."""
  return abi.bind_library(lib, HEADER_PATH)


# Everything below is READ from include/easyrec_hip.h (abi.py): the header is the only place a record or a constant is
# stated.  The records, under the names the package uses:
LookupDesc = abi.RECORDS['er_lookup_desc']
OptHyper = abi.RECORDS['er_opt_hyper']
GradTerm = abi.RECORDS['er_grad_term']
GradGroup = abi.RECORDS['er_grad_group']  # (its `lambda` is `lam` here)
KvJob = abi.RECORDS['er_kv_job']
KvRouteJob = abi.RECORDS['er_kv_route_job']
CeHead = abi.RECORDS['er_ce_head']
TailJob = abi.RECORDS['er_tail_job']
LossTailJob = abi.RECORDS['er_loss_tail_job']
DenseOptJob = abi.RECORDS['er_dense_opt_job']
GemmProblem = abi.RECORDS['er_gemm_problem']
BnLayer = abi.RECORDS['er_bn_layer']
CastDesc = abi.RECORDS['er_cast_desc']
GemmEpilogue = abi.RECORDS['er_gemm_epilogue']
ColsumJob = abi.RECORDS['er_colsum_job']
DenseApplyDesc = abi.RECORDS['er_dense_apply_desc']
(COMBINER_SUM, COMBINER_MEAN, COMBINER_SQRTN, OPT_SGD, OPT_ADAM, OPT_LAZY_ADAM, OPT_ADAGRAD, ACT_NONE, ACT_RELU,
 BN_NONE, BN_BATCH, BN_FROZEN, GEMM_NN, GEMM_NT, GEMM_TN, EPI_PLAIN, EPI_STATS, EPI_BN_BWD, EPI_CROSS_FWD, EPI_CROSS_BWD,
 GRAD_TERM_ROWSUM, GRAD_TERM_FM, FRONT_SKIP_ONE_ROW, FRONT_DEFER_CATCH_UP, ABI_VERSION) = (
     abi.CONSTANTS['ER_' + name] for name in (
         'COMBINER_SUM', 'COMBINER_MEAN', 'COMBINER_SQRTN', 'OPT_SGD', 'OPT_ADAM', 'OPT_LAZY_ADAM', 'OPT_ADAGRAD', 'ACT_NONE',
         'ACT_RELU', 'BN_NONE', 'BN_BATCH', 'BN_FROZEN', 'GEMM_NN', 'GEMM_NT', 'GEMM_TN', 'EPI_PLAIN', 'EPI_STATS',
         'EPI_BN_BWD', 'EPI_CROSS_FWD', 'EPI_CROSS_BWD', 'GRAD_TERM_ROWSUM', 'GRAD_TERM_FM', 'FRONT_SKIP_ONE_ROW',
         'FRONT_DEFER_CATCH_UP', 'ABI_VERSION'))
COMBINERS = {'sum': COMBINER_SUM, 'mean': COMBINER_MEAN, 'sqrtn': COMBINER_SQRTN}
# er_opt_hyper as the flat float array the host writes: its length and the index of each field
HYPER_FLOATS = ctypes.sizeof(OptHyper) // 4
HYPER_LR, HYPER_LR_T, HYPER_BETA1, HYPER_BETA2, HYPER_OMB1, HYPER_OMB2, HYPER_EPS, HYPER_GSCALE, HYPER_CLIP = (
    getattr(OptHyper, f).offset // 4 for f in ('lr', 'lr_t', 'beta1', 'beta2', 'one_minus_beta1', 'one_minus_beta2', 'eps',
                                               'grad_scale', 'clip_scale'))


_wgrad_tls = threading.local()
_bn_tls = threading.local()


def take_last_bn_source():
  """The BnSource of the LinearBNActFn that just ran on this thread (None when the fused path is off)."""
  src, _bn_tls.last = getattr(_bn_tls, 'last', None), None
  return src


class WgradSink(object):
  """Weight gradients queued during one backward pass (HipBackend.defer_wgrads / flush_wgrads)."""

  def __init__(self):
    self.active = False
    self.queue = []
    self.queue_bf16 = []  # (a bf16 step's weight gradients: er_gemm_grouped_bf16)
    # bias gradients left as per-row-tile column sums by the fused cross backward [(partial [T, ld], dst [n], n)]:
    # finished by ONE launch when the backward pass is over (HipBackend.take_wgrads -> colsum_partials_multi)
    self.colsum_jobs = []

  # a bf16 step's weight gradients dW = x^T . dz contract over the BATCH: their operands are k-strided in HBM, which the bf16
  # kernel with operands in HBM (er_gemm_bf16_nt) does not take, and er_gemm_grouped_bf16 rounds fp32 operands while staging
  # them (122 us per DCN-v2 step for what the fp32 launch inside the step's fused tail does in the shadow of the embedding
  # update).  Default: the fp32 contraction of the fp32 activations / gradients the step holds anyway - the weight
  # gradient is then the one quantity of a bf16 step computed at HIGHER precision; '0' = er_gemm_grouped_bf16.
  bf16_wgrad_f32 = os.environ.get('EASYREC_AMD_BF16_WGRAD_F32', '1') != '0'

  def put(self, x, dy, out, bf16):
    if not self.active:
      return False
    (self.queue_bf16 if (bf16 and not self.bf16_wgrad_f32) else self.queue).append((x, dy, out, None, True))
    return True


class BnSource(object):
  """What the dgrad GEMM of a consumer needs in order to emit, in its epilogue, the BatchNorm-backward column sums
  of the layer that produced its input (HipBackend.gemm_bn_bwd): that layer's z, y and batch statistics."""
  __slots__ = ('z', 'zbias', 'y', 'mean', 'invstd', 'act', 'partial', 'dx_ptr', 'gamma', 'grad_bufs', 'beta', 'fused', 'pending',
               'frozen', 'dz_done')

  def __init__(self, z, zbias, y, mean, invstd, act, gamma=None, grad_bufs=None, beta=None, fused=True):
    assert y is not None
    self.z, self.zbias, self.y, self.mean, self.invstd, self.act = z, zbias, y, mean, invstd, act
    self.partial, self.dx_ptr = None, 0
    self.gamma, self.grad_bufs = gamma, grad_bufs  # grad_bufs = (gamma.grad, beta.grad) slices of the flat buffer
    # fused: the consumer's dgrad GEMM may emit this layer's BatchNorm-backward column sums (HipBackend.fused_bn_bwd)
    self.beta, self.fused = beta, fused
    # pending: the layer's BatchNorm finalize + apply has NOT been launched yet (LinearBNActFn(defer_apply=True)): y, mean,
    # invstd are unwritten until the ONE consumer the model promised runs it (WideFmConcatFn: er_bn_apply_wide_fm) or
    # finish_pending_bn does; holds the arguments of HipBackend.bn_apply_from_stats
    self.pending = None
    # frozen: the layer normalises with the MOVING statistics (its backward is elementwise); dz_done: the contraction that
    # produced this layer's dy has already turned it into dz (er_gemm_problem.bn_dz_out, GroupedLinearFn.backward)
    self.frozen, self.dz_done = False, False


class BnColsView(object):
  """`src`'s layer output as the column block [col0, col0 + width) of a wider tensor (DeepFM's [sum(wide) | FM | deep]):
  the consumer's dgrad GEMM emits that layer's BatchNorm-backward column sums from those columns of its output
  (HipBackend.gemm_bn_bwd(col0=...))."""
  __slots__ = ('src', 'col0', 'ref')
  fused = True  # (what LinearBNActFn.forward asks of a BnSource)

  def __init__(self, src, col0, ref):
    self.src, self.col0, self.ref = src, int(col0), ref


def tag_bn_cols(joined, part, col0):
  """`joined[:, col0:col0 + part.shape[1]]` is a copy of `part`, the output of a fused dense + BatchNorm layer."""
  src = bn_source_of(part)
  if src is not None and src.fused:
    joined._er_bn_cols = BnColsView(src, col0, joined)
  return joined


def bn_cols_of(x):
  """The BnColsView of x if x IS the untouched tensor tag_bn_cols marked (dense + BatchNorm layers take it as `src`)."""
  if not getattr(hip(), 'bn_cols_epilogue', False):
    return None
  v = getattr(x, '_er_bn_cols', None)
  if v is None or x.dim() != 2 or x.data_ptr() != v.ref.data_ptr() or x.shape != v.ref.shape or x.stride() != v.ref.stride():
    return None
  return v


def tag_bn_source(y, src):
  """Mark `y` (what the layer function returns) as the output described by src."""
  y._er_bn_src = src
  return y


def grad_sink_of(x, col0=0, width=None):
  """The GradSink of x if x IS a group output of the embedding engine (layers/input_layer.py) and a deposit into
  columns [col0, col0 + width) is allowed now, else None."""
  sink = getattr(x, '_er_sink', None)
  if sink is None or x.dim() != 2:
    return None
  return sink


def grad_slots_of_step():
  """The step's gradient-slot table (kernels.grad_slot), or None: taken in a Function's FORWARD and kept on its ctx - the
  backward may run on an autograd worker thread, where the thread-local model context is not set."""
  from easyrec_amd.core import context
  stack = context._stack()
  return getattr(stack[-1], 'grad_slots', None) if (stack and _GRAD_SLOTS) else None


_GRAD_SLOTS = os.environ.get('EASYREC_AMD_GRAD_SLOTS', '1') != '0'  # A/B switch
_CAT_DGRAD = os.environ.get('EASYREC_AMD_CAT_DGRAD', '1') != '0'    # A/B switch: one input-gradient GEMM for the readers of a shared input


class _SlotGateFn(torch.autograd.Function):
  """Identity.  Every SLOT-AWARE consumer of an activation reads it through ONE gate per step (slot_gate), so the gate's
  backward - which autograd runs only after all of THEM - is where their shared gradient buffer enters x's gradient."""

  @staticmethod
  def forward(ctx, x):
    # (when every consumer deposited its gradient elsewhere - an embedding group's GradSink - nothing arrives here: without
    # this autograd would materialise a zero tensor and the group would add it to its buffer: a fill + an axpy2d for nothing)
    ctx.set_materialize_grads(False)
    return x.view_as(x)

  @staticmethod
  def backward(ctx, g):
    return g


def slot_gate(x):
  """The tensor a slot-aware Function (LinearFn, CrossV2EpilogueFn, DINConcatFn, DINPoolFn) must be APPLIED to instead of
  x.  grad_slot lets those consumers accumulate their input gradients into one buffer that the first of them returns to
  autograd.  If that buffer went to x directly, an ordinary consumer of x (a torch op, LinearBNActFn, ...) whose gradient
  arrives between two slot consumers would make autograd sum out of place - buffer + other - and the later slot consumers
  would add into a buffer nobody reads any more.  Behind the gate the buffer is the ONLY gradient autograd sees for the gate's
  output, complete when the gate's backward hands it on to x, whatever else reads x and in whatever order."""
  slots = grad_slots_of_step()
  if slots is None or not torch.is_grad_enabled() or not x.requires_grad or x.dim() < 2:
    return x
  gates = slots.setdefault('gates', {})
  key = (x.data_ptr(), tuple(x.shape), tuple(x.stride()))
  ent = gates.get(key)
  if ent is not None and (ent[0] is x or ent[1] is x):
    return ent[1]
  if ent is not None and x._base is not None and ent[0]._base is x._base and ent[0]._version == x._version and \
      ent[0].dtype == x.dtype:
    # another VIEW OBJECT of the same activation with the same geometry (dense() on a 3-D input reshapes it on every call):
    # its consumers must share the first view's gate - grad_slot keys the shared buffer by storage start and shape, and two
    # gates over one buffer would let the first hand it to autograd while the second's consumers are still adding into it.
    # The gradient reaches the common base through the first view's node: the same values.
    return ent[1]
  xg = _SlotGateFn.apply(x)
  for attr in ('_er_bn_src', '_er_sink'):
    if hasattr(x, attr):
      setattr(xg, attr, getattr(x, attr))
  gates[key] = (x, xg)
  return xg


def grad_slot(slots, x):
  """One gradient buffer per activation tensor and step, shared by the backward kernels of ALL its slot-aware consumers: the
  first to ask gets (a fresh tensor, accumulate = False, first = True) and returns that tensor to autograd; the others get
  (the same tensor, True, False), ADD into it inside their own kernels and return None - autograd then has one gradient for
  x and launches no add kernel.  The consumers must have been applied to slot_gate(x): see there.  Keyed by storage start
  and shape; the table (grad_slots_of_step) is emptied by EasyRecModel.begin_step."""
  key = (x.data_ptr(), tuple(x.shape))
  t = slots.get(key)
  if t is not None:
    return t, True, False
  t = torch.empty(x.shape, dtype=torch.float32, device=x.device)
  slots[key] = t
  return t, False, True


def bn_source_of(x):
  """The BnSource of x if x IS the untouched 2-D output of a fused dense + BatchNorm + activation layer."""
  src = getattr(x, '_er_bn_src', None)
  if src is None:
    return None
  ref = src.y
  if x.dim() != 2 or x.data_ptr() != ref.data_ptr() or x.shape != ref.shape or x.stride() != ref.stride():
    return None
  return src


CROSS_HASH_KEY = 0xDECAFCAFFE  # tf.sparse.cross_hashed's default hash_key (crossed_column(hash_key=None))


def same_lookup_keys(group, leader):
  """Do two table groups see the same keys every step (er_emb_group_share_sort's condition)?"""
  if group is leader or leader.get('sort_leader') is not None:
    return False
  a, b = group['specs'], leader['specs']
  if len(a) != len(b) or group.get('n_active', -1) != leader.get('n_active', -1):
    return False
  for k in ('world', 'shard_stride', 'local_base'):
    if group.get(k) != leader.get(k):
      return False
  for x, y in zip(a, b):
    if (_p(x.ids), _p(x.offsets), x.rows, x.key_base, x.n_rows, x.max_nnz) != \
        (_p(y.ids), _p(y.offsets), y.rows, y.key_base, y.n_rows, y.max_nnz):
      return False
  return True


@dataclass
class LookupSpec:
  """One embedding lookup (tensor-level view of er_lookup_desc).

  table:   [rows, dim] fp32 view of the lookup's table inside its table group
  ids:     int64 [n_rows] (dense mode, id < 0 = missing) or [max_nnz] (ragged mode)
  offsets: None or int32 [n_rows + 1]
  weights: None or fp32, aligned with ids
  out:     2-D fp32 base tensor [n_rows, out_stride]; forward output or upstream gradient
  """
  table: torch.Tensor
  ids: torch.Tensor
  offsets: Optional[torch.Tensor]
  weights: Optional[torch.Tensor]
  out: torch.Tensor
  out_col: int
  rows: int
  key_base: int
  dim: int
  combiner: int
  n_rows: int
  max_nnz: int
  name: str = ''

  def with_out(self, out):
    return LookupSpec(self.table, self.ids, self.offsets, self.weights, out, self.out_col,
                      self.rows, self.key_base, self.dim, self.combiner, self.n_rows,
                      self.max_nnz, self.name)


def _p(t):
  return None if t is None else t.data_ptr()


def _np(a):
  return a.ctypes.data


def _stream():
  return torch.cuda.current_stream().cuda_stream


def _f32c(t, name='tensor'):
  assert t.dtype == torch.float32 and t.is_contiguous(), '%s must be contiguous fp32' % name
  return t


class Bf16Shadows(object):
  """dense_dtype 'bf16' (BASELINE config 3): the bf16 operands the contractions read from HBM.

  Weights: two bf16 shadows per fp32 master in `varstore.flat` - `plain` [K, pad8(N)] (the k-contiguous operand of the
  input-gradient product dx = dy . W^T) and `t` [N, pad8(K)] (of the forward product x . W) - written by ONE er_cast_bf16
  launch after every dense optimizer step (HipBackend.dense_opt_step) and whenever the store's weights were replaced
  (VarStore.version).  Activations: cast by act() when a contraction needs them (their producers write fp32)."""

  def __init__(self, be, varstore):
    import weakref
    self.be = be
    self.vs = weakref.ref(varstore)
    flat = varstore.flat
    self.lo, self.hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * 4
    self.device = flat.device
    self.weights = {}  # data_ptr -> (master view [K, N], plain, t)
    self.seen_version = getattr(varstore, 'version', 0)
    # per step (begin_step): bf16 copies of fp32 activations / gradients that their PRODUCER wrote beside the fp32 tensor
    # (BatchNorm apply, the cross epilogue, concat, the BatchNorm backward: register) or that an earlier contraction of
    # the forward pass cast (act(cache=True)): (data_ptr, shape, stride) -> (the fp32 tensor, kept alive so that its
    # address cannot be handed out again within the step; its bf16 copy)
    self.copies = {}

  def begin_step(self):
    self.copies = {}

  @staticmethod
  def _key(x):
    return (x.data_ptr(), tuple(x.shape), tuple(x.stride()))

  def register(self, x, xb):
    self.copies[self._key(x)] = (x, xb)

  def new_copy(self, x):
    """An empty bf16 buffer [rows, pad8(cols)] for a producer to fill beside the fp32 matrix x (the padding columns are
    read as the k-tail of a contraction: zeroed here when there are any), registered as x's copy."""
    rows, cols = x.shape
    pc = self.pad8(cols)
    xb = torch.empty(rows, pc, dtype=torch.bfloat16, device=x.device) if pc == cols else \
        torch.zeros(rows, pc, dtype=torch.bfloat16, device=x.device)
    self.register(x, xb)
    return xb

  @staticmethod
  def pad8(n):
    return (int(n) + 7) // 8 * 8

  def owns(self, t):
    return self.lo <= t.data_ptr() < self.hi

  def alive(self):
    return self.vs() is not None

  def _descs(self, entries):
    return [d for w, plain, t in entries for d in ((w, plain, False), (w, t, True))]

  def weight(self, w):
    vs = self.vs()
    if vs is not None and getattr(vs, 'version', 0) != self.seen_version:
      self.refresh()
    e = self.weights.get(w.data_ptr())
    if e is None or e[0].shape != w.shape:
      K, N = w.shape
      plain = torch.zeros(K, self.pad8(N), dtype=torch.bfloat16, device=self.device)
      t = torch.zeros(N, self.pad8(K), dtype=torch.bfloat16, device=self.device)
      e = self.weights[w.data_ptr()] = (w.detach(), plain, t)
      self.be.cast_bf16(self._descs([e]))
    return e

  def refresh(self):
    vs = self.vs()
    if vs is not None:
      self.seen_version = getattr(vs, 'version', 0)
    if self.weights:
      self.be.cast_bf16(self._descs(self.weights.values()))

  def act(self, x, transpose=False, cache=False):
    """A bf16 copy of the fp32 matrix x ([rows, pad8(cols)], or its transpose [cols, pad8(rows)]): the one its producer
    registered, else a cast launch.  cache: x will not change any more within the step (a forward activation) - later
    contractions reuse this cast."""
    if not transpose:
      e = self.copies.get(self._key(x))
      if e is not None:
        return e[1]
    rows, cols = x.shape
    dst = torch.empty((cols, self.pad8(rows)) if transpose else (rows, self.pad8(cols)), dtype=torch.bfloat16,
                      device=x.device)
    self.be.cast_bf16([(x, dst, transpose)])
    if cache and not transpose:
      self.register(x, dst)
    return dst


class _CheckedCalls(object):
  """`ck.er_NAME(...)` calls `lib.er_NAME(...)` and hands a non-zero return code to `fail(rc, 'er_NAME')`: the name in
  the error is the name of the function that was called.  For the entry points that return 0 or an error; those that
  return a value or a code the caller interprets are called through `lib`."""

  def __init__(self, lib, fail):
    self._lib, self._fail = lib, fail

  def __getattr__(self, name):  # (the first use of a name only: the callable then is an attribute of its own)
    fn, fail = getattr(self._lib, name), self._fail

    def call(*args):
      rc = fn(*args)
      if rc != 0:
        fail(rc, name)
    setattr(self, name, call)
    return call


class HipBackend(object):
  """Tensor-level wrappers.  Every method launches asynchronously on torch's current stream."""

  name = 'hip'

  def __init__(self):
    self._adopt(load_library(LIB_PATH))
    if self.lib.er_abi_version() != ABI_VERSION:
      raise RuntimeError('easyrec_amd: ABI version mismatch in %s' % LIB_PATH)

  def _adopt(self, bound_lib):
    self._lib, self.ck = bound_lib, _CheckedCalls(bound_lib, self._ck)

  @property
  def lib(self):
    return self._lib

  @lib.setter
  def lib(self, lib):
    # a library opened elsewhere (a host-only backend made without __init__) is bound here: every wrapper passes plain
    # Python values, which an unbound CDLL would truncate to C ints
    self._adopt(bind_library(lib))

  # -- measurement hook (bench.py): with `op_log` a list, every contraction appends (kernel name as rocprof prints it,
  # flops): one eager step gives the algorithmic work behind each GEMM kernel of the step's profile
  op_log = None
  _LAYOUT_TPL = {GEMM_NN: '<true, false>', GEMM_NT: '<true, true>', GEMM_TN: '<false, false>'}

  def _log_gemm(self, kernel, layout, M, N, K):
    if self.op_log is not None:
      self.op_log.append(('er::' + kernel + (self._LAYOUT_TPL[int(layout)] if layout is not None else ''),
                          2.0 * M * N * K))

  # -- plumbing
  def _ck(self, rc, what):
    if rc != 0:
      msg = self.lib.er_last_error()
      raise RuntimeError('%s failed (rc=%d): %s' % (what, rc, msg.decode() if msg else ''))

  @staticmethod
  def require_device():
    if not torch.cuda.is_available():
      raise RuntimeError('easyrec_amd: no HIP device visible; the training path needs an MI355X '
                         '(there is no CPU fallback).')

  def reserve_scratch(self, floats):
    self.ck.er_reserve_scratch(int(floats))

  def config_set(self, key, value):
    self.ck.er_config_set(key.encode(), int(value))

  def device_info(self):
    cu, wave = ctypes.c_int(0), ctypes.c_int(0)
    buf = ctypes.create_string_buffer(64)
    self.ck.er_device_info(ctypes.byref(cu), ctypes.byref(wave), buf, 64)
    return {'cu_count': cu.value, 'wave_size': wave.value, 'arch': buf.value.decode()}

  # -- K14 sharded embedding checkpoint files (host code)
  def save_dense_embed(self, ckpt_path, var_name, task_index, task_num, vals_np):
    vals_np = np.ascontiguousarray(vals_np, dtype=np.float32)
    rows, dim = vals_np.shape
    self.ck.er_save_dense_embed(ckpt_path.encode(), var_name.encode(), task_index, task_num,
                                _np(vals_np), rows, dim)

  def load_dense_embed(self, ckpt_path, var_name, task_index, task_num, embed_dim, embed_part_size):
    out = np.empty((embed_part_size, embed_dim), dtype=np.float32)
    n = ctypes.c_int64(0)
    self.ck.er_load_dense_embed(ckpt_path.encode(), var_name.encode(), task_index, task_num, embed_dim,
                                embed_part_size, _np(out), ctypes.byref(n))
    return out

  def load_kv_embed(self, ckpt_path, var_name, task_index, task_num, embed_dim):
    n = ctypes.c_int64(0)
    args = (ckpt_path.encode(), var_name.encode(), task_index, task_num, embed_dim)
    self.ck.er_load_kv_embed(*args, 0, None, None, ctypes.byref(n))
    keys = np.empty(n.value, dtype=np.int64)
    vals = np.empty((n.value, embed_dim), dtype=np.float32)
    if n.value:
      self.ck.er_load_kv_embed(*args, n.value, _np(keys), _np(vals), ctypes.byref(n))
    return keys, vals

  # -- K1 hashing
  def decode_csv_host(self, text, sep, kinds, max_rows, threads=0, out=None):
    """CSVInput's decode step on the host.  text: uint8 array; kinds: 0 string / 1 int / 2 float per field.  threads: 0 =
    one per hardware thread (at most 8), n > 1 = that many (er_decode_csv_host_mt); 1 = the single-pass form
    (er_decode_csv_host).  out: a dict the five output arrays are kept in between calls of the same shape (for a reader
    that is done with a batch's arrays before it decodes the next: fresh 1.3 MB arrays are page-faulted in on every call).
    Returns (n_rows, consumed bytes, ints [F, max_rows], floats, empty mask, str_begin, str_len)."""
    text = np.ascontiguousarray(text, dtype=np.uint8)
    kinds = np.ascontiguousarray(kinds, dtype=np.int32)
    F = len(kinds)
    # (the threaded decoder writes its column-major outputs at a pitch that is not a power of two: a row's F fields x 5
    # arrays at a 4096-element pitch share their cache sets; the arrays handed back are [F, max_rows] views)
    pitch = max_rows if int(threads) == 1 else max_rows + 24
    key = (F, int(max_rows), int(pitch))
    if out is not None and out.get('key') == key:
      ints, flts, empty, begin, length = out['arrays']
    else:
      ints = np.empty((F, pitch), dtype=np.int64)[:, :max_rows]
      flts = np.empty((F, pitch), dtype=np.float64)[:, :max_rows]
      empty = np.empty((F, pitch), dtype=np.uint8)[:, :max_rows]
      begin = np.empty((F, pitch), dtype=np.int64)[:, :max_rows]
      length = np.empty((F, pitch), dtype=np.int32)[:, :max_rows]
      if out is not None:
        out['key'], out['arrays'] = key, (ints, flts, empty, begin, length)
    n_rows, consumed = ctypes.c_int64(0), ctypes.c_int64(0)
    sep_b = sep.encode('utf-8') if isinstance(sep, str) else bytes(sep)
    assert len(sep_b) == 1, 'separator must be one byte: %r' % sep

    if text.size == 0:
      return 0, 0, ints, flts, empty, begin, length
    if int(threads) == 1:
      self.ck.er_decode_csv_host(_np(text), text.size, sep_b[0], F,
                                 _np(kinds), int(max_rows), _np(ints), _np(flts), _np(empty),
                                 _np(begin), _np(length), ctypes.byref(n_rows), ctypes.byref(consumed))
    else:
      self.ck.er_decode_csv_host_mt(_np(text), text.size, sep_b[0], F,
                                    _np(kinds), int(max_rows), int(pitch), _np(ints),
                                    _np(flts), _np(empty), _np(begin), _np(length), ctypes.byref(n_rows),
                                    ctypes.byref(consumed), int(threads))
    return n_rows.value, consumed.value, ints, flts, empty, begin, length

  def pack_cells_host(self, text, begin, length):
    """Cells (begin, length) of `text` -> (packed uint8 bytes, int64 offsets[n + 1])."""
    text = np.ascontiguousarray(text, dtype=np.uint8)
    begin = np.ascontiguousarray(begin, dtype=np.int64)
    length = np.ascontiguousarray(length, dtype=np.int32)
    n = len(begin)
    out = np.empty(max(int(length.sum(dtype=np.int64)), 1), dtype=np.uint8)
    offsets = np.empty(n + 1, dtype=np.int64)
    self.ck.er_pack_cells_host(_np(text if text.size else out), _np(begin), _np(length), n,
                               _np(out), _np(offsets))
    return out[:int(offsets[-1])], offsets

  def split_cells_host(self, text, begin, length, seps, keep_empty=False, max_tokens=0):
    """Cells (begin, length) of `text` split on the bytes of `seps` -> (tok_begin int64 [T], tok_len int32 [T],
    row_offsets int64 [n + 1]) (er_split_cells_host)."""
    text = np.ascontiguousarray(text, dtype=np.uint8)
    begin = np.ascontiguousarray(begin, dtype=np.int64)
    length = np.ascontiguousarray(length, dtype=np.int32)
    n = len(begin)
    cap = int(length.sum(dtype=np.int64)) + n + 1
    tb, tl = np.empty(cap, dtype=np.int64), np.empty(cap, dtype=np.int32)
    offs = np.empty(n + 1, dtype=np.int64)
    sb = np.frombuffer(seps if isinstance(seps, bytes) else seps.encode('utf-8'), dtype=np.uint8)
    self.ck.er_split_cells_host(_np(text if text.size else tb), _np(begin), _np(length), n, _np(sb),
                                len(sb), keep_empty, int(max_tokens), _np(tb), _np(tl), cap, _np(offs))
    T = int(offs[-1])
    return tb[:T], tl[:T], offs

  def pack_int_decimal_host(self, values):
    """int64 array -> (packed uint8 bytes, int64 offsets[n + 1]) of the values' decimal strings (str(int))."""
    values = np.ascontiguousarray(values, dtype=np.int64).reshape(-1)
    n = values.size
    out = np.empty(max(20 * n, 1), dtype=np.uint8)
    offsets = np.empty(n + 1, dtype=np.int64)
    self.ck.er_pack_int_decimal_host(_np(values), n, _np(out), _np(offsets))
    return out[:int(offsets[-1])], offsets

  def sparse_cross_hashed_host(self, bytes_np, offsets_np, n_rows, n_cols, num_buckets, hash_key=None):
    """ComboFeature through crossed_column: column-major strings -> int64 [n_rows] bucket ids ('' is a value too)."""
    bytes_np = np.ascontiguousarray(bytes_np, dtype=np.uint8)
    offsets_np = np.ascontiguousarray(offsets_np, dtype=np.int64)
    assert len(offsets_np) == n_rows * n_cols + 1
    out = np.empty(n_rows, dtype=np.int64)
    if bytes_np.size == 0:
      bytes_np = np.zeros(1, dtype=np.uint8)
    key = CROSS_HASH_KEY if hash_key is None else int(hash_key)
    self.ck.er_sparse_cross_hashed_host(_np(bytes_np), _np(offsets_np), int(n_rows), int(n_cols), int(num_buckets),
                                        key, _np(out))
    return out

  def hash_bucket_fast_host(self, bytes_np, offsets_np, n_per_col, num_buckets, drop_empty):
    """numpy in / numpy out; runs on the host (data-loader threads)."""
    bytes_np = np.ascontiguousarray(bytes_np, dtype=np.uint8)
    offsets_np = np.ascontiguousarray(offsets_np, dtype=np.int64)
    nb = np.ascontiguousarray(num_buckets, dtype=np.uint64)
    n = len(offsets_np) - 1
    out = np.empty(n, dtype=np.int64)
    if bytes_np.size == 0:
      bytes_np = np.zeros(1, dtype=np.uint8)
    self.ck.er_hash_bucket_fast_host(_np(bytes_np), _np(offsets_np), n, int(n_per_col), _np(nb), int(drop_empty),
                                     _np(out))
    return out

  def hash_bucket_fast(self, bytes_t, offsets_t, n_per_col, num_buckets_t, drop_empty, out=None):
    n = offsets_t.numel() - 1
    if out is None:
      out = torch.empty(n, dtype=torch.int64, device=bytes_t.device)
    self.ck.er_hash_bucket_fast(_p(bytes_t), _p(offsets_t), n, int(n_per_col), _p(num_buckets_t), int(drop_empty),
                                _p(out), _stream())
    return out

  def hash_bucket_fast_int64(self, values_t, n_per_col, num_buckets_t, out=None):
    n = values_t.numel()
    if out is None:
      out = torch.empty(n, dtype=torch.int64, device=values_t.device)
    self.ck.er_hash_bucket_fast_int64(_p(values_t), n, int(n_per_col),
                                      _p(num_buckets_t), _p(out), _stream())
    return out

  # -- K2 / K3 / K4 embeddings
  @staticmethod
  def _descs(specs):
    arr = (LookupDesc * len(specs))()
    for i, s in enumerate(specs):
      assert s.table.dtype == torch.float32 and s.ids.dtype == torch.int64
      assert s.out.dim() == 2 and s.out.stride(1) == 1
      d = arr[i]
      d.table = s.table.data_ptr()
      d.ids = s.ids.data_ptr()
      d.offsets = s.offsets.data_ptr() if s.offsets is not None else None
      d.weights = s.weights.data_ptr() if s.weights is not None else None
      d.out = s.out.data_ptr()
      d.rows, d.key_base, d.dim = s.rows, s.key_base, s.dim
      d.out_stride, d.out_col, d.combiner = s.out.stride(0), s.out_col, s.combiner
      d.n_rows, d.max_nnz = s.n_rows, s.max_nnz
      # a column block of a wider buffer as the table (er_emb_fwd only: rows received side by side with another group's)
      assert s.table.dim() != 2 or s.table.stride(1) == 1
      d.table_ld = s.table.stride(0) if (s.table.dim() == 2 and s.table.stride(0) != s.dim) else 0
    return arr

  def emb_plan_create(self, specs):
    plan = ctypes.c_void_p(0)
    self.ck.er_emb_plan_create(self._descs(specs), len(specs), ctypes.byref(plan))
    nblk = self.lib.er_emb_plan_num_blocks(plan)
    return {'handle': plan, 'specs': list(specs), 'num_blocks': nblk}

  def emb_plan_destroy(self, plan):
    self.lib.er_emb_plan_destroy(plan['handle'])

  def emb_fwd(self, plan, sumsq_partials=None):
    self.ck.er_emb_fwd(plan['handle'], _p(sumsq_partials), _stream())

  def emb_group_create(self, specs, dim, total_rows, var, m, v, bitmap):
    grp = ctypes.c_void_p(0)
    self.ck.er_emb_group_create(self._descs(specs), len(specs), dim, total_rows, _p(var), _p(m), _p(v), _p(bitmap),
                                ctypes.byref(grp))
    n_ent = self.lib.er_emb_group_num_entries(grp)
    group = {'handle': grp, 'specs': list(specs), 'dim': dim, 'total_rows': total_rows, 'var': var,
             'm': m, 'v': v, 'bitmap': bitmap, 'num_entries': n_ent, 'last_step': None}
    self._set_row_pitch(group)
    return group

  def _set_row_pitch(self, group):
    """var / m / v (and last_step) may be column blocks of ONE [rows, ld] record buffer (input_layer._alloc_storage):
    the pitches are read off the tensors' strides."""
    var, ls = group['var'], group.get('last_step')
    ld = var.stride(0) if var.dim() == 2 else group['dim']
    for t in (group['m'], group['v']):
      assert t is None or (t.dim() == 2 and t.stride(0) == ld and t.stride(1) == 1), 'var / m / v must share one row pitch'
    assert var.dim() != 2 or var.stride(1) == 1
    ls_ld = 1 if ls is None else (ls.stride(0) if ls.numel() > 1 else 1)
    if ld != group['dim'] or ls_ld != 1:
      self.ck.er_emb_group_set_row_pitch(group['handle'], ld, ls_ld)

  def emb_group_tile_entries(self, group):
    """Entries of the key-sorted list per workgroup of the backward (runs that cross a multiple of it take the fix launch)."""
    return int(self.lib.er_emb_group_tile_entries(group['handle']))

  def emb_group_destroy(self, group):
    self.lib.er_emb_group_destroy(group['handle'])

  def emb_bwd_update(self, group, opt_kind, hyper):
    self.ck.er_emb_bwd_update(group['handle'], opt_kind, _p(hyper), _stream())

  def emb_bwd_reduce(self, group, out=None):
    """out: a (keys, grads, n_unique) triple from an earlier call to reuse (fixed addresses for hipGraphs)."""
    n = group['num_entries']
    dev = group['var'].device
    if out is None:
      keys = torch.empty(n, dtype=torch.int32, device=dev)
      grads = torch.empty(n, group['dim'], dtype=torch.float32, device=dev)
      n_unique = torch.zeros(1, dtype=torch.int32, device=dev)
    else:
      keys, grads, n_unique = out
    self.ck.er_emb_bwd_reduce(group['handle'], _p(keys), _p(grads), _p(n_unique), _stream())
    return keys, grads, n_unique

  # -- K13 GEMM on the matrix cores
  def gemm_reserve(self, floats):
    self.ck.er_gemm_reserve(int(floats))

  def gemm_row_tiles(self, M):
    return int(self.lib.er_gemm_row_tiles(int(M)))

  def bn_apply_from_stats(self, x, bias, col_stats, chunks, gamma, beta, eps, momentum, moving_mean, moving_var, act,
                          bf16_state=None):
    """BatchNorm(train) + activation from ready-made column statistics (er_gemm's epilogue).  bf16_state (a Bf16Shadows):
    the launch also writes y's bf16 copy, registered there for the contraction that reads y next."""
    B, N = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(N, dtype=torch.float32, device=x.device)
    invstd = torch.empty(N, dtype=torch.float32, device=x.device)
    yb = bf16_state.new_copy(y) if bf16_state is not None else None
    self.ck.er_bn_apply_from_stats_b16(_p(_f32c(x)), _p(bias), _p(col_stats), int(chunks), _p(gamma), _p(beta), B,
                                       N, eps, momentum, _p(moving_mean), _p(moving_var), int(act), _p(y),
                                       _p(mean), _p(invstd), _p(yb), 0 if yb is None else yb.stride(0),
                                       _stream())
    return y, mean, invstd

  def gemm(self, layout, a, b, out=None, bias=None, accumulate=False, bf16=False, col_stats=None):
    """out (+)= op(a) . op(b) (+ bias).  2-D fp32 tensors with unit inner stride.
    layout GEMM_NN: a[M,K] b[K,N]; GEMM_NT: a[M,K] b[N,K]; GEMM_TN: a[K,M] b[K,N]."""
    assert a.dim() == 2 and b.dim() == 2 and a.stride(1) == 1 and b.stride(1) == 1
    assert a.dtype == torch.float32 and b.dtype == torch.float32
    if layout == GEMM_NN:
      (M, K), (K2, N) = a.shape, b.shape
    elif layout == GEMM_NT:
      (M, K), (N, K2) = a.shape, b.shape
    else:
      (K, M), (K2, N) = a.shape, b.shape
    assert K == K2, 'gemm: inner dimensions %d vs %d' % (K, K2)
    if out is None:
      assert not accumulate
      out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    assert out.shape == (M, N) and out.stride(1) == 1 and out.dtype == torch.float32
    if bf16 and self._gemm_bf16_fast(layout, a, b, out, bias, accumulate, M, N, K, col_stats=col_stats):
      return out
    if layout == GEMM_NN and not bf16 and not accumulate and col_stats is None and self.gemv_ok(a, M, N, K):
      return self._gemv(a, None, b, bias, out)
    self._log_gemm('gemm_bf16_kernel' if bf16 else 'gemm_f32_kernel', layout, M, N, K)
    fn = self.ck.er_gemm_bf16 if bf16 else self.ck.er_gemm_f32
    if col_stats is not None:
      assert col_stats.numel() >= self.gemm_row_tiles(M) * N * 3 and col_stats.dtype == torch.float32
    fn(layout, M, N, K, _p(a), a.stride(0), _p(b), b.stride(0), _p(out), out.stride(0), _p(bias), accumulate,
       _p(col_stats), _stream())
    return out

  # -- bf16 operands in HBM (dense_dtype 'bf16'): er_gemm_bf16_nt
  bf16_nt = True  # (False: er_gemm_bf16, which converts fp32 operands while staging - round 1's form, kept for tests)

  # the producers of a bf16 step write their consumers' bf16 operands and the bf16 contractions carry the BatchNorm /
  # cross epilogues (er_gemm_bf16_nt_epi); A/B switch: '0' = round 5's arrangement (cast launches, fp32-only epilogues)
  bf16_epilogues = os.environ.get('EASYREC_AMD_BF16_EPILOGUES', '1') != '0'

  def bf16_enable(self, varstore):
    """Called by the estimator (dense_dtype 'bf16') once the dense variables are packed; outside graph capture."""
    self.ck.er_gemm_bf16_nt_prepare()
    states = [s for s in getattr(self, '_bf16_states', []) if s.alive()]
    st = Bf16Shadows(self, varstore)
    states.append(st)
    self._bf16_states = states
    return st

  def _bf16_state_of(self, t):
    for st in getattr(self, '_bf16_states', ()):
      if st.owns(t) and st.alive():
        return st
    return None

  def cast_bf16(self, items):
    """items: [(src fp32 [rows, cols] (unit inner stride), dst bf16, transpose)]: dst[r, c] = src[r, c] or
    dst[c, r] = src[r, c], padding columns of dst zeroed; ceil(n / 16) launches."""
    n = len(items)
    arr = (CastDesc * n)()
    for i, (src, dst, tr) in enumerate(items):
      assert src.dim() == 2 and src.stride(1) == 1 and src.dtype == torch.float32
      assert dst.dim() == 2 and dst.stride(1) == 1 and dst.dtype == torch.bfloat16
      rows, cols = src.shape
      assert dst.shape[0] == (cols if tr else rows) and dst.stride(0) >= (rows if tr else cols)
      arr[i] = CastDesc(src.data_ptr(), dst.data_ptr(), rows, cols, src.stride(0), dst.stride(0), 1 if tr else 0)
    self.ck.er_cast_bf16(arr, n, _stream())

  def gemm_bf16_nt(self, a, bt, M, N, K, out=None, out_bf16=None, bias=None, accumulate=False, epi=None):
    """out[M, N] (+)= a[M, K] . bt[N, K]^T (+ bias): bf16 operands with leading dimensions that are multiples of 8,
    fp32 accumulate; out fp32 and / or out_bf16.  epi: a GemmEpilogue record (er_gemm_bf16_nt_epi)."""
    assert a.dtype == torch.bfloat16 and bt.dtype == torch.bfloat16 and a.stride(1) == 1 and bt.stride(1) == 1
    assert a.shape[0] >= M and bt.shape[0] >= N
    Kp = (K + 7) // 8 * 8  # (the k-tail up to the padded width reads zeros: Bf16Shadows pads with zeros)
    assert a.stride(0) >= Kp and bt.stride(0) >= Kp and a.stride(0) % 8 == 0 and bt.stride(0) % 8 == 0
    kind = EPI_PLAIN if epi is None else int(epi.kind)
    self._log_gemm('gemm_bf16_nt_kernel<4, %d>' % kind, None, M, N, K)
    self.ck.er_gemm_bf16_nt_epi(M, N, Kp, _p(a), a.stride(0), _p(bt), bt.stride(0), _p(out),
                                0 if out is None else out.stride(0), _p(out_bf16),
                                0 if out_bf16 is None else out_bf16.stride(0), _p(bias), accumulate,
                                None if epi is None else ctypes.byref(epi), _stream())
    return out

  @staticmethod
  def _nt_rows_ok(*ts):
    """The epilogues of er_gemm_bf16_nt_epi read / write fp32 rows in 16-byte pieces."""
    return all(t is None or (t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0 and t.stride(1) == 1) for t in ts)

  def _gemm_bf16_fast(self, layout, a, b, out, bias, accumulate, M, N, K, col_stats=None):
    """The bf16 contraction through er_gemm_bf16_nt when one operand is a weight of a bf16-enabled store (forward
    x . W, input gradient dy . W^T); False = not applicable.  col_stats: the following BatchNorm's per-row-tile column
    statistics from the epilogue (ER_EPI_STATS)."""
    if not self.bf16_nt or layout == GEMM_TN:
      return False
    st = self._bf16_state_of(b)
    if st is None:
      return False
    epi = None
    if col_stats is not None:
      if N % 4 != 0 or accumulate or not self._nt_rows_ok(out):
        return False
      epi = GemmEpilogue(kind=EPI_STATS, col_stats=col_stats.data_ptr())
    w, plain, t = st.weight(b)
    a16 = st.act(a, cache=(layout == GEMM_NN))
    self.gemm_bf16_nt(a16, t if layout == GEMM_NN else plain, M, N, K, out=out, bias=bias, accumulate=accumulate, epi=epi)
    return True

  # er_gemm_f32_bn_bwd / er_bn_act_bwd_from_partials are used
  fused_bn_bwd = True
  # the BatchNorm-backward column sums of a layer whose output is a column block of the consumer's input (DeepFM's deep
  # tower inside [sum(wide) | FM | deep]) from the consumer's dgrad epilogue (er_gemm_f32_bn_bwd_cols); A/B switch
  bn_cols_epilogue = os.environ.get('EASYREC_AMD_BN_COLS_EPILOGUE', '1') != '0'

  def gemm_bn_bwd(self, layout, a, b, src, partial, col0=None, bf16=False):
    """dgrad GEMM whose epilogue also emits the BatchNorm-backward column sums of the layer described by `src`
    (a BnSource: the producer of this GEMM's input) into partial [row tiles][N][2].  col0: that layer produced the
    columns [col0, col0 + its width) of this GEMM's input only.  bf16: through er_gemm_bf16_nt_epi (ER_EPI_BN_BWD) when
    b is a weight of a bf16-enabled store; None = not applicable there."""
    assert a.dim() == 2 and b.dim() == 2 and a.stride(1) == 1 and b.stride(1) == 1
    if layout == GEMM_NN:
      (M, K), (K2, N) = a.shape, b.shape
    elif layout == GEMM_NT:
      (M, K), (N, K2) = a.shape, b.shape
    else:
      (K, M), (K2, N) = a.shape, b.shape
    if bf16:
      st = self._bf16_state_of(b) if (self.bf16_nt and layout == GEMM_NT) else None
      n_src = src.y.shape[1]
      c0 = 0 if col0 is None else int(col0)
      if st is None or N % 4 or n_src % 4 or c0 % 4 or not self._nt_rows_ok(src.z, src.y) or src.y.stride() != src.z.stride():
        return None
      assert K == K2 and src.z.shape == (M, n_src) and c0 + n_src <= N and partial.numel() >= self.gemm_row_tiles(M) * n_src * 2
      out = torch.empty(M, N, dtype=torch.float32, device=a.device)
      epi = GemmEpilogue(kind=EPI_BN_BWD, bn_z=src.z.data_ptr(), bn_zbias=_p(src.zbias), bn_y=src.y.data_ptr(),
                         bn_mean=_p(src.mean), bn_invstd=_p(src.invstd), bn_partial=partial.data_ptr(),
                         bn_ld=src.y.stride(0), bn_use_bn=int(src.mean is not None), bn_act=int(src.act), bn_col0=c0,
                         bn_n_src=n_src)
      w, plain, t = st.weight(b)
      self.gemm_bf16_nt(st.act(a), plain, M, N, K, out=out, epi=epi)
      return out
    if col0 is not None:
      n_src = src.y.shape[1]
      assert K == K2 and src.z.shape == (M, n_src) and src.y.stride() == src.z.stride() and 0 <= col0 and col0 + n_src <= N
      assert partial.numel() >= self.gemm_row_tiles(M) * n_src * 2
      self._log_gemm('gemm_f32_bn_bwd_kernel', layout, M, N, K)
      out = torch.empty(M, N, dtype=torch.float32, device=a.device)
      self.ck.er_gemm_f32_bn_bwd_cols(layout, M, N, K, _p(a), a.stride(0), _p(b), b.stride(0), _p(out),
                                      out.stride(0), _p(src.z), _p(src.zbias), _p(src.y), _p(src.mean),
                                      _p(src.invstd), src.y.stride(0), int(src.mean is not None),
                                      int(src.act), _p(partial), int(col0), n_src, _stream())
      return out
    assert K == K2 and src.z.shape == (M, N) and src.y.shape == (M, N) and src.y.stride() == src.z.stride()
    assert partial.numel() >= self.gemm_row_tiles(M) * N * 2
    self._log_gemm('gemm_f32_bn_bwd_kernel', layout, M, N, K)
    out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    use_bn = src.mean is not None
    self.ck.er_gemm_f32_bn_bwd(layout, M, N, K, _p(a), a.stride(0), _p(b), b.stride(0), _p(out),
                               out.stride(0), _p(src.z), _p(src.zbias), _p(src.y), _p(src.mean),
                               _p(src.invstd), src.y.stride(0), int(use_bn), int(src.act), _p(partial),
                               _stream())
    return out

  # the same-depth layers of parallel stacks (MMoE's experts, task towers) as one grouped launch: layers/dnn.py run_parallel
  grouped_stacks = True

  # the bias / BatchNorm / activation launches of those layers as one launch forward, two backward (er_bn_fwd_multi /
  # er_bn_bwd_multi)
  grouped_bn = True
  BN_MULTI_MAX_ROWS = 8192  # (taller layers reduce their partial sums in a merge launch of their own: single launches)

  def bn_fwd_multi(self, layers):
    """layers: [dict(x, bias, gamma, beta, moving_mean, moving_var, col_stats, use_bn, act, eps, momentum)] -> [(y, mean,
    invstd)]: the forward of BNFromStatsFn (use_bn 1: batch statistics from the GEMM's epilogue) / BNActFn (0, BN_FROZEN)
    for all of them in ONE launch."""
    arr = (BnLayer * len(layers))()
    outs = []
    for q, l in zip(arr, layers):
      x = l['x']
      assert x.dim() == 2 and x.is_contiguous() and x.dtype == torch.float32 and x.shape[0] <= self.BN_MULTI_MAX_ROWS
      B, N = x.shape
      y = torch.empty_like(x)
      mean = torch.empty(N, dtype=torch.float32, device=x.device) if l['use_bn'] else None
      invstd = torch.empty(N, dtype=torch.float32, device=x.device) if l['use_bn'] else None
      q.x, q.bias, q.gamma, q.beta = x.data_ptr(), _p(l.get('bias')), _p(l.get('gamma')), _p(l.get('beta'))
      q.moving_mean, q.moving_var = _p(l.get('moving_mean')), _p(l.get('moving_var'))
      q.B, q.N, q.use_bn, q.act = B, N, int(l['use_bn']), int(l['act'])
      q.eps, q.momentum = float(l.get('eps', 0.0)), float(l.get('momentum', 0.0))
      if int(l['use_bn']) == BN_BATCH:
        q.col_stats, q.chunks = l['col_stats'].data_ptr(), self.gemm_row_tiles(B)
      q.y, q.save_mean, q.save_invstd = y.data_ptr(), _p(mean), _p(invstd)
      outs.append((y, mean, invstd))
    self.ck.er_bn_fwd_multi(arr, len(layers), _stream())
    return outs

  def bn_bwd_multi(self, layers):
    """layers: [dict(x, bias, gamma, beta, y, mean, invstd, dy, use_bn, act, partial, into)] -> [(dx, dbias, dgamma, dbeta)]
    (bn_act_bwd's arguments and results, layer by layer) in two launches: column sums (of the layers without `partial`),
    finalize + apply."""
    arr = (BnLayer * len(layers))()
    outs = []
    for q, l in zip(arr, layers):
      x, dy = l['x'], l['dy']
      B, N = x.shape
      assert dy.dim() == 2 and dy.stride(1) == 1 and dy.dtype == torch.float32 and B <= self.BN_MULTI_MAX_ROWS
      dev = x.device
      dx_done = bool(l.get('dx_done'))  # (dy already holds dx: the contraction that produced it ran the elementwise backward)
      dx = dy if dx_done else torch.empty_like(x)
      into = l.get('into')
      if into is not None:
        dbias, dgamma, dbeta = into
      else:
        dbias = torch.empty(N, dtype=torch.float32, device=dev) if l.get('bias') is not None else None
        dgamma = torch.empty(N, dtype=torch.float32, device=dev) if l.get('gamma') is not None else None
        dbeta = torch.empty(N, dtype=torch.float32, device=dev) if l.get('gamma') is not None else None
      partial = l.get('partial')
      if partial is not None and dy.stride(0) != N:
        partial = None
      q.x, q.bias, q.gamma, q.beta = x.data_ptr(), _p(l.get('bias')), _p(l.get('gamma')), _p(l.get('beta'))
      q.B, q.N, q.use_bn, q.act = B, N, int(l['use_bn']), int(l['act'])
      q.save_mean, q.save_invstd = _p(l.get('mean')), _p(l.get('invstd'))
      q.y_in = _p(l['y'])
      q.dy, q.dy_ld = dy.data_ptr(), dy.stride(0)
      if partial is not None:
        q.partial, q.chunks = partial.data_ptr(), self.gemm_row_tiles(B)
      assert not dx_done or (partial is not None and int(l['use_bn']) == BN_FROZEN)
      q.dx, q.dbias, q.dgamma, q.dbeta = (None if dx_done else dx.data_ptr()), _p(dbias), _p(dgamma), _p(dbeta)
      q.accumulate = int(into is not None)
      outs.append((dx, None, None, None) if into is not None else (dx, dbias, dgamma, dbeta))
    self.ck.er_bn_bwd_multi(arr, len(layers), _stream())
    return outs

  def gemm_grouped(self, layout, problems, bf16=False):
    """problems: [(a, b, out, bias, accumulate)] fp32, one layout: ONE launch (+ one for the split-K reduces).
    bf16: operands rounded to bf16 while staged (er_gemm_grouped_bf16)."""
    arr = self._gemm_problems(layout, problems, bf16)
    if bf16:
      self.ck.er_gemm_grouped_bf16(layout, arr, len(problems), _stream())
    else:
      self.ck.er_gemm_grouped_f32(layout, arr, len(problems), _stream())

  def _gemm_problems(self, layout, problems, bf16=False, log_as=None):
    """The er_gemm_problem array of a grouped launch (log_as: the kernel the op log books the contractions under)."""
    arr = (GemmProblem * len(problems))()
    for q, pr in zip(arr, problems):
      a, b, out, bias, accumulate = pr[:5]
      stats = pr[5] if len(pr) > 5 else None
      bn = pr[6] if len(pr) > 6 else None  # (BnSource of the layer that produced this problem's output position, partial)
      assert a.dim() == 2 and b.dim() == 2 and a.stride(1) == 1 and b.stride(1) == 1 and out.stride(1) == 1
      assert a.dtype == torch.float32 and b.dtype == torch.float32 and out.dtype == torch.float32
      if layout == GEMM_NN:
        (M, K), (K2, N) = a.shape, b.shape
      elif layout == GEMM_NT:
        (M, K), (N, K2) = a.shape, b.shape
      else:
        (K, M), (K2, N) = a.shape, b.shape
      assert K == K2 and out.shape == (M, N)
      if self.op_log is not None:
        if log_as is not None:
          self._log_gemm(log_as, None, M, N, K)
        elif bf16:
          self._log_gemm('gemm_bf16_grouped_kernel', layout, M, N, K)
        else:
          self._log_gemm('gemm_f32_grouped_kernel', layout, M, N, K)
      q.M, q.N, q.K = M, N, K
      q.A, q.lda, q.B, q.ldb = a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0)
      q.C, q.ldc = out.data_ptr(), out.stride(0)
      q.bias = bias.data_ptr() if bias is not None else None
      q.accumulate = int(bool(accumulate))
      if stats is not None:
        assert stats.dtype == torch.float32 and stats.numel() >= self.gemm_row_tiles(M) * N * 3 and not accumulate
        q.col_stats = stats.data_ptr()
      if bn is not None:
        src, partial = bn[:2]
        if len(bn) > 2 and bn[2]:  # (the layer's elementwise backward in this launch's epilogue: frozen statistics only)
          assert src.frozen and layout == GEMM_NT
          q.bn_gamma, q.bn_dz_out = _p(src.gamma), 1
        assert src.z.shape == (M, N) and partial.numel() >= self.gemm_row_tiles(M) * N * 2 and not accumulate
        q.bn_z, q.bn_zbias = _p(src.z), _p(src.zbias)
        q.bn_y = _p(src.y)
        q.bn_mean, q.bn_invstd = _p(src.mean), _p(src.invstd)
        q.bn_ld, q.bn_use_bn, q.bn_act = src.z.stride(0), int(src.mean is not None), int(src.act)
        q.bn_partial = partial.data_ptr()
      fz = pr[7] if len(pr) > 7 else None  # (the frozen-BatchNorm forward epilogue: er_gemm_problem.fz_*)
      if fz is not None:
        assert layout == GEMM_NN and not bf16 and stats is None and bn is None and not accumulate
        y, save = fz['y'], fz['save']
        assert y.shape == (M, N) and y.stride(0) == out.stride(0) and y.stride(1) == 1 and save.is_contiguous() and \
            save.numel() == 2 * N
        q.fz_bias, q.fz_gamma, q.fz_beta = _p(fz.get('bias')), _p(fz.get('gamma')), _p(fz.get('beta'))
        q.fz_mean, q.fz_var = fz['moving_mean'].data_ptr(), fz['moving_var'].data_ptr()
        q.fz_eps, q.fz_act = float(fz['eps']), int(fz['act'])
        q.fz_y, q.fz_save = y.data_ptr(), save.data_ptr()
    return arr

  # weight gradients of a backward pass: queued by LinearFn / LinearBNActFn, contracted together by flush_wgrads()
  def wgrad_sink(self):
    """The calling thread's queue object.  Functions fetch it in forward() (the caller's thread: the simulated ranks
    of the embedding-parallel tests are threads) because backward() runs on an autograd engine thread."""
    sink = getattr(_wgrad_tls, 'sink', None)
    if sink is None:
      sink = _wgrad_tls.sink = WgradSink()
    return sink

  def defer_wgrads(self):
    sink = self.wgrad_sink()
    assert not sink.queue and not sink.queue_bf16, 'flush_wgrads() was not called for the previous backward pass'
    sink.active = True

  def flush_wgrads(self):
    """Launch the queued weight gradients on the current stream.  Returns the queue: when that stream is not the one
    the operands were produced on, the caller keeps it alive until the streams have joined."""
    q, qb = self.take_wgrads()
    if q:
      self.gemm_grouped(GEMM_TN, q)
    if qb:
      self.gemm_grouped(GEMM_TN, qb, bf16=True)
    return q + qb

  def take_wgrads(self):
    """The queued weight gradients (fp32, bf16), NOT launched: the caller contracts them - the fused tail puts the fp32
    ones into the embedding backward's grid (emb_bwd_fused(wgrads=...))."""
    sink = self.wgrad_sink()
    q, sink.queue, sink.active = sink.queue, [], False
    qb, sink.queue_bf16 = sink.queue_bf16, []
    jobs, sink.colsum_jobs = sink.colsum_jobs, []
    if jobs:
      self.colsum_partials_multi(jobs)
    return q, qb

  def queue_colsum(self, sink, partial, dst, n_cols):
    """dst[j] += sum_p partial[p, j] once the backward pass is over (one launch for all queued jobs), or now."""
    if sink is not None and sink.active:
      sink.colsum_jobs.append((partial, dst, n_cols))
    else:
      self.colsum_partials_multi([(partial, dst, n_cols)])

  @staticmethod
  def colsum_is_narrow(x):
    """er_colsum_acc would take its one-workgroup-per-column form for x"""
    return x.dim() == 2 and x.shape[1] <= 8 and x.shape[0] * x.shape[1] <= (1 << 17) and x.stride(1) == 1

  def colsum_narrow_multi(self, jobs, accumulate=True):
    """jobs: [(x [rows, cols <= 8], out [cols])]: out[j] (+)= sum_i x[i, j], all jobs in ONE launch (column by column the
    sums of colsum())."""
    arr = (ColsumJob * len(jobs))()
    for q, (x, out) in zip(arr, jobs):
      assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == torch.float32 and out.is_contiguous() and out.numel() == x.shape[1]
      q.x, q.rows, q.cols, q.x_stride, q.out = x.data_ptr(), x.shape[0], x.shape[1], x.stride(0), out.data_ptr()
    self.ck.er_colsum_narrow_multi(arr, len(jobs), accumulate, _stream())

  def colsum_partials_multi(self, jobs, accumulate=True):
    """jobs: [(partial [P, ld], dst [n_cols], n_cols)]: dst[j] (+)= sum_p partial[p, j], all jobs in one launch."""
    arr = (TailJob * len(jobs))()
    for q, (partial, d, n_cols) in zip(arr, jobs):
      assert partial.dim() == 2 and partial.stride(1) == 1 and d.is_contiguous() and d.numel() == n_cols
      q.partial, q.dst, q.n_parts, q.n_cols, q.ld = partial.data_ptr(), d.data_ptr(), partial.shape[0], int(n_cols), partial.stride(0)
    self.ck.er_colsum_partials_multi(arr, len(jobs), accumulate, _stream())

  # the step's tail in one grid (er_emb_bwd_fused_wgrad); A/B switch, and the workgroups its contraction's k-splits aim at
  # (0: the stand-alone launch's 512 - bit-identical to the unfused tail; same-box 256 -> 54.5 us, 512 -> 60, 1024 -> 66)
  fused_tail = os.environ.get('EASYREC_AMD_FUSED_TAIL', '1') != '0'
  tail_wgrad_blocks = int(os.environ.get('EASYREC_AMD_TAIL_BLOCKS', '256'))

  @staticmethod
  def wgrads_fit_the_tail(q):
    """plain fp32 contractions only, at most one grouped launch's worth"""
    return 0 < len(q) <= 16 and all(len(pr) <= 5 for pr in q)

  # -- K12 embedding-parallel routing (include/easyrec_hip.h)
  def emb_group_set_routing(self, group, world, shard_stride, local_base):
    arr = (ctypes.c_int64 * len(local_base))(*[int(x) for x in local_base])
    self.ck.er_emb_group_set_routing(group['handle'], world, shard_stride, arr)
    group['world'], group['shard_stride'], group['local_base'] = world, shard_stride, list(local_base)

  def emb_group_set_active(self, group, n_rows):
    self.ck.er_emb_group_set_active(group['handle'], int(n_rows))
    group['n_active'] = int(n_rows)

  def emb_group_share_sort(self, group, leader):
    """True when `group` now reuses `leader`'s per-step sort (identical ids and table geometry), else False."""
    if not same_lookup_keys(group, leader):
      return False
    self.ck.er_emb_group_share_sort(group['handle'], leader['handle'])
    group['sort_leader'] = leader
    return True

  def emb_route(self, group, unique_keys, n_unique, entry_unique_index, owner_counts):
    if unique_keys is None:  # follower of a shared sort: the outputs are the leader's
      assert group.get('sort_leader') is not None and n_unique is None and entry_unique_index is None
      self.ck.er_emb_route(group['handle'], None, None, None, None, _stream())
      return
    assert unique_keys.dtype == torch.int32 and n_unique.dtype == torch.int32
    assert entry_unique_index is None or entry_unique_index.dtype == torch.int64
    assert owner_counts is None or owner_counts.dtype == torch.int32
    self.ck.er_emb_route(group['handle'], _p(unique_keys), _p(n_unique), _p(entry_unique_index),
                         _p(owner_counts), _stream())

  def emb_bwd_reduce_routed(self, group, unique_grads):
    assert unique_grads.dtype == torch.float32 and unique_grads.dim() == 2 and unique_grads.stride(1) == 1
    self.ck.er_emb_bwd_reduce_routed(group['handle'], _p(unique_grads), unique_grads.stride(0),
                                     _stream())

  # the embedding-parallel requester's local reductions + the step's weight gradients + the loss tail as two launches
  # (er_emb_reduce_local_tail); A/B switch: '0' = one launch per reduction kind and dim group, the grouped wgrad launch apart
  ep_merged_reduce = os.environ.get('EASYREC_AMD_EP_MERGED_REDUCE', '1') != '0'

  def emb_reduce_local_tail(self, routed, dense, wgrads=None):
    """routed: [(sharded requester group, unique_grads [slots, >= dim])], dense: [(replicated group, dense [rows, dim + 1])]
    (at most 4 together): their local gradient reductions in ONE tile launch + ONE fix launch; wgrads: take_wgrads()'s fp32
    list (wgrads_fit_the_tail) contracted in the same grid, with a deferred loss tail (loss_tail(defer=True)) as one more
    workgroup of it."""
    items = [(g, 1, t) for g, t in routed] + [(g, 2, t) for g, t in dense]
    n = len(items)
    assert 1 <= n <= 4
    for _, _, t in items:
      assert t.dim() == 2 and t.stride(1) == 1 and t.dtype == torch.float32
    gh = (ctypes.c_void_p * n)(*[g['handle'] for g, _, _ in items])
    modes = (ctypes.c_int32 * n)(*[m for _, m, _ in items])
    outs = (ctypes.c_void_p * n)(*[t.data_ptr() for _, _, t in items])
    ld = (ctypes.c_int32 * n)(*[t.stride(0) for _, _, t in items])
    pr, lt = None, None
    if wgrads:
      pr = self._gemm_problems(GEMM_TN, wgrads, log_as='emb_reduce_local_wgrad_kernel')
      lt = self._deferred_loss_tail
      self._deferred_loss_tail = None
    self.ck.er_emb_reduce_local_tail(gh, modes, outs, ld, n, pr, len(wgrads) if wgrads else 0,
                                     int(self.tail_wgrad_blocks) if wgrads else 0,
                                     ctypes.byref(lt[0]) if lt is not None else None, _stream())

  def gather_rows(self, table, keys, n, key_sub, out):
    assert keys.dtype == torch.int32 and table.dim() == 2 and table.stride(1) == 1
    self.ck.er_gather_rows_ld(_p(table), table.stride(0), table.shape[0], table.shape[1], _p(keys), int(n),
                              int(key_sub), _p(out), _stream())

  def scatter_unique(self, keys, grads, n_unique, capacity, dim, dense):
    assert dense.dim() == 2 and dense.stride(1) == 1
    self.ck.er_scatter_unique(_p(keys), _p(grads), _p(n_unique), int(capacity),
                              dim, _p(dense), dense.stride(0), _stream())

  def emb_owner_merge(self, group, run_counts):
    """Owner side: the received keys are len(run_counts) ascending duplicate-free runs; merge instead of sort."""
    n = len(run_counts)
    rc = (ctypes.c_int32 * n)(*[int(x) for x in run_counts])
    self.ck.er_emb_owner_merge(group['handle'], rc, n, _stream())

  def emb_group_set_peer_capacity(self, group, peer_cap, count_header=True):
    self.ck.er_emb_group_set_peer_capacity(group['handle'], int(peer_cap), 1 if count_header else 0)
    group['peer_cap'], group['peer_hdr'] = int(peer_cap), bool(count_header)

  def emb_route_overflow(self, group):
    out = ctypes.c_int32(0)
    self.ck.er_emb_route_overflow(group['handle'], ctypes.byref(out))
    return bool(out.value)

  def emb_owner_ids(self, recv_keys, counts, n_runs, peer_cap, key_sub, ids, counts_out):
    """counts None: the received runs carry their count in front ([count, keys ...], peer_cap + 1 slots each)."""
    hdr = 1 if counts is None else 0
    assert recv_keys.dtype == torch.int32 and ids.dtype == torch.int64 and counts_out.dtype == torch.int32
    assert recv_keys.numel() >= n_runs * (peer_cap + hdr) and ids.numel() >= n_runs * peer_cap and counts_out.numel() >= n_runs
    assert counts is None or (counts.dtype == torch.int32 and counts.numel() >= n_runs)
    self.ck.er_emb_owner_ids(_p(recv_keys), None if counts is None else _p(counts), n_runs, int(peer_cap),
                             int(key_sub), _p(ids), _p(counts_out), _stream())

  # owner ids + entry build + merge (+ the serve launch's lag-1 replay table) as one launch - A/B switch
  ep_owner_fused = os.environ.get('EASYREC_AMD_EP_OWNER_FUSED', '1') != '0'

  def emb_owner_ids_merge(self, group, recv_keys, n_runs, peer_cap, key_sub, ids, counts_out, build_tables):
    """er_emb_owner_ids_merge: emb_owner_ids (runs with their count in front) + emb_owner_merge_padded in one launch."""
    assert recv_keys.dtype == torch.int32 and ids.dtype == torch.int64 and counts_out.dtype == torch.int32
    assert recv_keys.numel() >= n_runs * (peer_cap + 1) and ids.numel() >= n_runs * peer_cap and counts_out.numel() >= n_runs
    self.ck.er_emb_owner_ids_merge(group['handle'], _p(recv_keys), None, n_runs, int(peer_cap), int(key_sub),
                                   _p(ids), _p(counts_out), 1 if build_tables else 0, _stream())

  def emb_owner_merge_padded(self, group, counts, n_runs, peer_cap):
    assert counts.dtype == torch.int32 and counts.numel() >= n_runs
    self.ck.er_emb_owner_merge_padded(group['handle'], _p(counts), n_runs,
                                      int(peer_cap), _stream())

  def emb_owner_serve(self, groups, rows_out, hyper):
    """Catch up (lazy dense decay) and reply the received rows of up to 4 owner groups in one launch."""
    n = len(groups)
    gh = (ctypes.c_void_p * n)(*[g['handle'] for g in groups])
    for g, o in zip(groups, rows_out):  # (a column block of a wider buffer is fine: ld = its row stride)
      assert o.stride(1) == 1 and o.dtype == torch.float32 and o.shape[1] == g['dim']
    op = (ctypes.c_void_p * n)(*[o.data_ptr() for o in rows_out])
    ld = (ctypes.c_int32 * n)(*[o.stride(0) for o in rows_out])
    self.ck.er_emb_owner_serve(gh, op, ld, n, None if hyper is None else _p(hyper), _stream())

  def emb_bwd_reduce_dense(self, groups, dense):
    """Per-row gradient sums of the groups straight into their dense [rows, dim + 1] buffers (count in the last
    column); one launch for all groups."""
    n = len(groups)
    for d in dense:
      assert d.dim() == 2 and d.stride(1) == 1 and d.dtype == torch.float32
    gh = (ctypes.c_void_p * n)(*[g['handle'] for g in groups])
    dp = (ctypes.c_void_p * n)(*[d.data_ptr() for d in dense])
    ld = (ctypes.c_int32 * n)(*[d.stride(0) for d in dense])
    self.ck.er_emb_bwd_reduce_dense(gh, dp, ld, n, _stream())

  def emb_dense_apply(self, tables, opt_kind, hyper):
    """tables: [(var, m, v, dense)] - one pass over each replicated table after the all-reduce of `dense`."""
    n = len(tables)
    descs = (DenseApplyDesc * n)()
    for i, (var, m, v, dense) in enumerate(tables):
      assert var.stride(1) == 1 and dense.stride(1) == 1 and dense.shape[0] == var.shape[0]
      assert all(t is None or t.stride() == var.stride() for t in (m, v))
      descs[i] = DenseApplyDesc(var.data_ptr(), None if m is None else m.data_ptr(), None if v is None else v.data_ptr(),
                                dense.data_ptr(), dense.stride(0), var.shape[1], var.shape[0], var.stride(0))
    self.ck.er_emb_dense_apply(descs, n, opt_kind, _p(hyper), _stream())

  def emb_mark_touched(self, group):
    self.ck.er_emb_mark_touched(group['handle'], _stream())

  def emb_sweep_untouched(self, group, hyper):
    self.ck.er_emb_sweep_untouched(group['handle'], _p(hyper), _stream())

  def stream_copy(self, src, dst):
    nbytes = src.numel() * src.element_size()
    assert dst.numel() * dst.element_size() >= nbytes
    self.ck.er_stream_copy(_p(src), _p(dst), nbytes, _stream())

  def adam_decay_sweep(self, var, m, v, bitmap, total_rows, dim, hyper):
    ld = var.stride(0) if var.dim() == 2 else dim
    assert var.dim() != 2 or (m.stride() == var.stride() and v.stride() == var.stride() and var.stride(1) == 1)
    self.ck.er_adam_decay_sweep_ld(_p(var), _p(m), _p(v), _p(bitmap), total_rows, dim, ld, _p(hyper), _stream())

  # -- K5 FM / wide
  def fm_fwd(self, x, F, D):
    """x: [B, >=F*D] row-major (stride(0) = row stride).  Returns (fm [B,D], S [B,D])."""
    B = x.shape[0]
    fm = torch.empty(B, D, dtype=torch.float32, device=x.device)
    S = torch.empty(B, D, dtype=torch.float32, device=x.device)
    self.ck.er_fm_fwd(_p(x), B, F, D, x.stride(0), _p(fm), _p(S), _stream())
    return fm, S

  def fm_bwd(self, x, S, g, F, D, into=None, accumulate=False):
    B = x.shape[0]
    dx = torch.empty(B, F * D, dtype=torch.float32, device=x.device) if into is None else into
    assert dx.shape == (B, F * D) and dx.stride(1) == 1
    self.ck.er_fm_bwd(_p(x), _p(S), _p(_f32c(g)), B, F, D, x.stride(0), _p(dx), dx.stride(0), int(accumulate),
                      _stream())
    return dx

  def auc_update(self, probs, labels, weights, thresholds, counts):
    """counts int64 [2, T + 1] += histogram of (label != 0, #thresholds below the prediction); see core/metrics.py."""
    probs, labels = _f32c(probs.reshape(-1)), _f32c(labels.reshape(-1))
    assert probs.numel() == labels.numel() and counts.dtype == torch.int64 and counts.is_contiguous()
    assert counts.numel() == 2 * (thresholds.numel() + 1)
    w = None if weights is None else _f32c(weights.reshape(-1))
    self.ck.er_auc_update(_p(probs), _p(labels), _p(w), probs.numel(), _p(thresholds),
                          thresholds.numel(), _p(counts), _stream())

  def grouped_auc(self, keys, preds, labels, reduction):
    """gAUC / session AUC of the accumulated rows (int64 keys, fp32 predictions, labels != 0 positive) -> (sum of
    w * AUC over the keys with both classes, sum of w, number of such keys); the ordering by (key, prediction) is two
    stable device sorts, the ranks and the reduction are er_grouped_auc (one host read at the end)."""
    n = keys.numel()
    preds, labels = _f32c(preds.reshape(-1)), _f32c(labels.reshape(-1))
    assert preds.numel() == n and labels.numel() == n and keys.dtype == torch.int64
    out = torch.zeros(3, dtype=torch.float64, device=keys.device)
    if n:
      by_pred = torch.sort(preds, stable=True).indices
      order = by_pred[torch.sort(keys.reshape(-1)[by_pred], stable=True).indices]
      k, p, y = keys.reshape(-1)[order].contiguous(), preds[order].contiguous(), labels[order].contiguous()
      work = torch.zeros(3 * n, dtype=torch.float64, device=keys.device)
      self.ck.er_grouped_auc(_p(k), _p(p), _p(y), n, int(reduction), _p(work), _p(out),
                             _stream())
    return tuple(float(x) for x in out.cpu().tolist())

  def dot_interaction_fwd(self, x, F, D, self_interaction, out=None):
    """x [B, >=F*D] (stride(0) = row stride) -> [B, P] pairwise dot products in the order of model/dlrm.py:51-57;
    `out`: a caller's [B, P] destination, rows out.stride(0) apart."""
    B = x.shape[0]
    P = F * (F - 1) // 2 + (F if self_interaction else 0)
    if out is None:
      out = torch.empty(B, P, dtype=torch.float32, device=x.device)
    assert x.dtype == torch.float32 and x.stride(1) == 1
    assert out.dtype == torch.float32 and out.shape == (B, P) and out.stride(1) == 1
    self.ck.er_dot_interaction_fwd(_p(x), B, F, D, x.stride(0), self_interaction, _p(out),
                                   out.stride(0), _stream())
    return out

  def dot_interaction_bwd(self, x, g, F, D, self_interaction, into=None, accumulate=False):
    """dx [B, F*D] of the pairwise dot products; x and g rows x.stride(0) / g.stride(0) apart; `into`: a caller's
    destination (rows into.stride(0) apart), written, or added to when `accumulate`."""
    B = x.shape[0]
    dx = torch.empty(B, F * D, dtype=torch.float32, device=x.device) if into is None else into
    assert x.dtype == torch.float32 and x.stride(1) == 1 and g.dtype == torch.float32 and g.stride(1) == 1
    assert dx.dtype == torch.float32 and dx.shape == (B, F * D) and dx.stride(1) == 1
    self.ck.er_dot_interaction_bwd(_p(x), _p(g), B, F, D, x.stride(0), self_interaction,
                                   g.stride(0), _p(dx), dx.stride(0), int(accumulate), _stream())
    return dx

  def rowsum_fwd(self, x, n):
    B = x.shape[0]
    out = torch.empty(B, 1, dtype=torch.float32, device=x.device)
    self.ck.er_rowsum_fwd(_p(x), B, n, x.stride(0), _p(out), _stream())
    return out

  fused_wide_fm = os.environ.get('EASYREC_AMD_FUSED_WIDE_FM', '1') != '0'  # A/B switch

  def wide_fm_concat(self, wide, fm_x, F, D, deep):
    """[sum(wide) | FM(fm_x) | deep] at a 16-byte row pitch and the FM field sums ([B, D]) in one launch."""
    B, n_w, n_d = wide.shape[0], wide.shape[1], deep.shape[1]
    assert wide.stride(1) == 1 and fm_x.stride(1) == 1 and deep.stride(1) == 1 and fm_x.shape[1] >= F * D
    width = 1 + D + n_d
    out = torch.empty(B, (width + 3) // 4 * 4, dtype=torch.float32, device=wide.device)[:, :width]
    S = torch.empty(B, D, dtype=torch.float32, device=wide.device)
    self.ck.er_wide_fm_concat(_p(wide), n_w, wide.stride(0), _p(fm_x), F, D, fm_x.stride(0), _p(deep), n_d,
                              deep.stride(0), B, _p(out), out.stride(0), _p(S), _stream())
    return out, S

  def bn_apply_wide_fm(self, pend, wide, fm_x, F, D):
    """er_bn_apply_wide_fm: the deferred BatchNorm finalize + apply `pend` (LinearBNActFn(defer_apply=True)) and
    [sum(wide) | FM(fm_x) | y] in ONE launch -> (out, S) as wide_fm_concat, or None when the library wants the two launches."""
    z, y = pend['z'], pend['y']
    B, N = z.shape
    n_w = wide.shape[1]
    assert wide.stride(1) == 1 and fm_x.stride(1) == 1 and fm_x.shape[1] >= F * D and z.is_contiguous() and y.is_contiguous()
    width = 1 + D + N
    out = torch.empty(B, (width + 3) // 4 * 4, dtype=torch.float32, device=wide.device)[:, :width]
    S = torch.empty(B, D, dtype=torch.float32, device=wide.device)
    rc = self.lib.er_bn_apply_wide_fm(_p(z), _p(pend['stats']), int(pend['chunks']), _p(pend['gamma']),
                                      _p(pend['beta']), B, N, pend['eps'], pend['momentum'],
                                      _p(pend['moving_mean']), _p(pend['moving_var']), int(pend['act']), _p(y),
                                      _p(pend['mean']), _p(pend['invstd']), _p(wide), n_w, wide.stride(0), _p(fm_x), F, D,
                                      fm_x.stride(0), _p(out), out.stride(0), _p(S), _stream())
    if rc == 3:
      return None
    self._ck(rc, 'er_bn_apply_wide_fm')
    return out, S

  def bn_apply_pending(self, pend):
    """the deferred BatchNorm finalize + apply as the launch of its own it would have been"""
    z = pend['z']
    B, N = z.shape
    self.ck.er_bn_apply_from_stats_b16(_p(z), None, _p(pend['stats']), int(pend['chunks']),
                                       _p(pend['gamma']), _p(pend['beta']), B, N, pend['eps'],
                                       pend['momentum'], _p(pend['moving_mean']),
                                       _p(pend['moving_var']), int(pend['act']), _p(pend['y']), _p(pend['mean']),
                                       _p(pend['invstd']), None, 0, _stream())

  # the last BatchNorm apply of DeepFM's deep tower inside the [sum(wide) | FM | deep] launch (er_bn_apply_wide_fm) - A/B switch
  defer_bn_apply = os.environ.get('EASYREC_AMD_DEFER_BN_APPLY', '1') != '0'

  # a TALL layer's BatchNorm apply inside the NEXT contraction's staging (er_bn_finalize_from_stats + er_gemm_f32_bn_a): the
  # [B * L, units] activations of DIN's attention MLP are not read back by an apply launch of their own - A/B switch
  bn_in_staging = os.environ.get('EASYREC_AMD_BN_IN_STAGING', '1') != '0'
  BN_IN_STAGING_MIN_ROWS = 256 * 64 + 1  # (layers whose column statistics take the merge launch: more than 256 row tiles)

  def bn_a_ok(self, pend, w):
    """May the deferred BatchNorm apply `pend` run inside the staging of the contraction with w [K, N]?"""
    z, y = pend['z'], pend['y']
    K = z.shape[1]
    return (K % 4 == 0 and K <= 256 and z.is_contiguous() and y.is_contiguous() and w.dim() == 2 and w.stride(1) == 1 and
            (z.data_ptr() | y.data_ptr()) % 16 == 0)

  # the bias + frozen BatchNorm + activation of a multi-task model's expert layers inside the grouped contraction's epilogue
  # (er_gemm_problem.fz_*: one launch writes z and y; the depth's BatchNorm launch disappears) - A/B switch
  frozen_bn_epilogue = os.environ.get('EASYREC_AMD_FROZEN_BN_EPILOGUE', '1') != '0'

  # ... and their elementwise backward (dz = gamma * invstd * masked dy) in the epilogue of the input-gradient contraction of
  # the layer ABOVE (er_gemm_problem.bn_dz_out): the experts' BatchNorm-backward passes of all but the last depth disappear
  frozen_dz_epilogue = os.environ.get('EASYREC_AMD_FROZEN_DZ_EPILOGUE', '1') != '0'

  # tall projections onto <= 4 columns (DIN's attention scores [B x L, 32] -> [B x L, 1]) by er_gemv_f32_bn_a - A/B switch
  tall_gemv = os.environ.get('EASYREC_AMD_TALL_GEMV', '1') != '0'

  def gemv_ok(self, x, M, N, K):
    return (self.tall_gemv and N <= 4 and M >= self.BN_IN_STAGING_MIN_ROWS and K % 4 == 0 and x.stride(1) == 1 and
            x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0)

  def _gemv(self, x, pend, w, bias, out=None):
    """out [M, N <= 4] = x . w (+ bias), or act(BatchNorm(z)) . w for a deferred apply `pend` (x = its z; statistics already
    finalized)"""
    M, K = x.shape
    N = w.shape[1]
    if out is None:
      out = torch.empty(M, N, dtype=torch.float32, device=x.device)
    if self.op_log is not None:
      self.op_log.append(('er::gemv_bna_kernel<%d>' % N, 2.0 * M * N * K))
    bn = pend is not None
    y = pend['y'] if bn else None
    self.ck.er_gemv_f32_bn_a(M, N, K, _p(x), x.stride(0), _p(pend['mean']) if bn else None,
                             _p(pend['invstd']) if bn else None, _p(pend['gamma']) if bn else None,
                             _p(pend['beta']) if bn else None, int(pend['act']) if bn else ACT_NONE, _p(y),
                             y.stride(0) if bn else 0, _p(w), w.stride(0), _p(out),
                             out.stride(0), _p(bias), _stream())
    return out

  def wgrad_tall_narrow_ok(self, x, dz):
    return (self.tall_gemv and x.dim() == 2 and dz.dim() == 2 and dz.shape[1] <= 4 and x.shape[0] >= self.BN_IN_STAGING_MIN_ROWS and
            x.shape[1] % 4 == 0 and x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0 and dz.stride(1) == 1 and
            x.dtype == torch.float32 and dz.dtype == torch.float32)

  def wgrad_tall_narrow(self, x, dz, out, accumulate=True, bias_grad=None):
    """out [K, N <= 4] (+)= x^T . dz for a tall x [rows, K] (er_wgrad_tall_narrow: the weight gradient of DIN's attention score
    projection, which stalled the grouped weight-gradient launch on its [rows, 1] operand)"""
    rows, K = x.shape
    N = dz.shape[1]
    assert out.shape == (K, N) and out.stride(1) == 1 and dz.shape[0] == rows
    assert bias_grad is None or (bias_grad.is_contiguous() and bias_grad.numel() == N)
    scratch = torch.empty(513 * (K + 1) * N, dtype=torch.float32, device=x.device)
    if self.op_log is not None:
      self.op_log.append(('er::wgrad_narrow_partial_kernel<%d>' % N, 2.0 * rows * N * K))
    self.ck.er_wgrad_tall_narrow(rows, K, N, _p(x), x.stride(0), _p(dz), dz.stride(0),
                                 _p(out), out.stride(0), _p(bias_grad), accumulate, _p(scratch),
                                 scratch.numel(), _stream())
    return out

  def gemm_bn_a(self, pend, w, bias, col_stats=None):
    """out [M, N] = act(BatchNorm(z)) . w (+ bias) for the deferred BatchNorm apply `pend` (LinearBNActFn(defer_apply=True)):
    the statistics are finalized by a launch of their own, the apply runs while the contraction stages its A tiles and leaves
    pend['y'] behind for the backward pass.  The same bits as bn_apply_pending + gemm."""
    z, y = pend['z'], pend['y']
    M, K = z.shape
    N = w.shape[1]
    self.ck.er_bn_finalize_from_stats(_p(pend['stats']), int(pend['chunks']), M, K,
                                      pend['eps'], pend['momentum'],
                                      _p(pend['moving_mean']), _p(pend['moving_var']), _p(pend['mean']),
                                      _p(pend['invstd']), _stream())
    if col_stats is None and self.gemv_ok(z, M, N, K):
      return self._gemv(z, pend, w, bias)
    out = torch.empty(M, N, dtype=torch.float32, device=z.device)
    if col_stats is not None:
      assert col_stats.numel() >= self.gemm_row_tiles(M) * N * 3 and col_stats.dtype == torch.float32
    self._log_gemm('gemm_f32_bna_kernel', None, M, N, K)
    self.ck.er_gemm_f32_bn_a(M, N, K, _p(z), z.stride(0), _p(pend['mean']), _p(pend['invstd']),
                             _p(pend['gamma']), _p(pend['beta']), int(pend['act']), _p(y),
                             y.stride(0), _p(w), w.stride(0), _p(out),
                             out.stride(0), _p(bias), _p(col_stats), _stream())
    return out

  def rowsum_bwd(self, g, n, into=None, accumulate=False):
    B = g.shape[0]
    dx = torch.empty(B, n, dtype=torch.float32, device=g.device) if into is None else into
    assert dx.shape == (B, n) and dx.stride(1) == 1
    self.ck.er_rowsum_bwd(_p(_f32c(g)), B, n, _p(dx), dx.stride(0), int(accumulate), _stream())
    return dx

  def group_grad_finish(self, groups):
    """groups: [(dout, out, lambda, has_base, [terms])], term = ('rowsum', g, col0, width) | ('fm', g, saved, col0,
    width, dim); g: [B] / [B, 1] / [B, dim] with unit inner stride.  One launch (er_group_grad_finish)."""
    arr, _keep = self._grad_groups(groups)
    self.ck.er_group_grad_finish(arr, len(groups), _stream())

  # the fused single-GPU embedding step: er_emb_front (build + sort + heads [+ decay table] in one launch, catch-up from
  # the heads) and er_emb_bwd_fused (finish + reduce + row update in one launch) - A/B switch
  fused_emb = os.environ.get('EASYREC_AMD_FUSED_EMB', '1') != '0'

  # the catch-up of lazy dense decay in registers (er_emb_fwd_lazy / er_emb_bwd_fused) instead of a launch of its own - A/B switch
  defer_catch_up = os.environ.get('EASYREC_AMD_DEFER_CATCH_UP', '1') != '0'

  def emb_front(self, groups, hyper, skip_one_row, defer=False):
    """-> False when the groups need the general path (nothing launched).  defer: no catch-up launch - the step's lookup
    must then be emb_fwd_lazy."""
    n = len(groups)
    gh = (ctypes.c_void_p * n)(*[g['handle'] for g in groups])
    flags = (FRONT_SKIP_ONE_ROW if skip_one_row else 0) | (FRONT_DEFER_CATCH_UP if defer else 0)
    rc = self.lib.er_emb_front(gh, n, flags, _p(hyper), _stream())
    if rc == 3:
      return False
    self._ck(rc, 'er_emb_front')
    return True

  def emb_fwd_lazy(self, plan, groups, hyper, sumsq_partials=None):
    """emb_fwd whose lookups into the lazily decaying `groups` catch their rows up in registers (after emb_front(defer))."""
    n = len(groups)
    gh = (ctypes.c_void_p * n)(*[g['handle'] for g in groups])
    self.ck.er_emb_fwd_lazy(plan['handle'], gh, n, _p(hyper), _p(sumsq_partials), _stream())

  def emb_front_fwd(self, groups, plan, hyper, skip_one_row, sumsq_partials=None):
    """emb_front(defer=True) + emb_fwd_lazy in one call (one launch when the prologue builds the replay table).
    -> False when the groups need the general path (nothing launched)."""
    n = len(groups)
    gh = (ctypes.c_void_p * n)(*[g['handle'] for g in groups])
    flags = (FRONT_SKIP_ONE_ROW if skip_one_row else 0) | FRONT_DEFER_CATCH_UP
    rc = self.lib.er_emb_front_fwd(gh, n, flags, plan['handle'], _p(hyper), _p(sumsq_partials), _stream())
    if rc == 3:
      return False
    self._ck(rc, 'er_emb_front_fwd')
    return True

  # the step's lag-1 replay table built by the prologue launch, so that sort and lookup share a launch - A/B switch
  prologue_tables = os.environ.get('EASYREC_AMD_PROLOGUE_TABLES', '1') != '0'

  def decay_tables_set_prologue_build(self, tabs, on):
    self.ck.er_decay_tables_set_prologue_build(tabs['handle'], on)
    tabs['prologue_build'] = bool(on)

  def decay_tables_sync(self, tabs):
    self.ck.er_decay_tables_sync(tabs['handle'], _stream())

  def decay_tables_error(self, tabs):
    flag = ctypes.c_int32(0)
    self.ck.er_decay_tables_error(tabs['handle'], ctypes.byref(flag))
    return bool(flag.value)

  def emb_bwd_fused(self, groups, finish, opt_kind, hyper, wgrads=None, dense_opt=None):
    """finish: group_grad_finish's descriptors, one per feature-group gradient buffer the groups' lookups write.
    wgrads: the step's queued weight gradients (take_wgrads()'s fp32 list, wgrads_fit_the_tail) - contracted in the same
    grid (er_emb_bwd_fused_tail), a deferred loss tail (loss_tail(defer=True)) as one more workgroup of it; dense_opt:
    dense_opt_step's arguments (w, m, v, grad, l2coef, opt_kind, hyper, l2_partials) - the dense optimizer behind the
    cross-tile fix, finishing the k-split weight gradients while it reads them (dense_opt_fits_the_tail).  Returns True
    when the optimizer ran here."""
    n = len(groups)
    gh = (ctypes.c_void_p * n)(*[g['handle'] for g in groups])
    arr, _keep = self._grad_groups(finish)
    if wgrads:
      pr = self._gemm_problems(GEMM_TN, wgrads, log_as='emb_bwd_own_wgrad_kernel')
      self.tail_launches = getattr(self, 'tail_launches', 0) + 1  # (tests: the fused tail is what ran)
      lt = self._deferred_loss_tail
      self._deferred_loss_tail = None
      oj = None
      if dense_opt is not None:
        w, m, v, grad, l2coef, kind, hyp, l2p = dense_opt
        oj = DenseOptJob(_p(w), _p(m), _p(v), _p(grad), _p(l2coef), w.numel(), int(kind), _p(hyp), _p(l2p))
      self.ck.er_emb_bwd_fused_tail(gh, n, arr, len(finish), opt_kind, _p(hyper), pr, len(wgrads),
                                    int(self.tail_wgrad_blocks),
                                    ctypes.byref(lt[0]) if lt is not None else None,
                                    ctypes.byref(oj) if oj is not None else None, _stream())
      if oj is not None:
        st = self._bf16_state_of(dense_opt[0])
        if st is not None:
          st.refresh()  # (a bf16 step whose dense optimizer ran in the tail: the weights' bf16 shadows follow the masters)
      return oj is not None
    self.ck.er_emb_bwd_fused(gh, n, arr, len(finish), opt_kind, _p(hyper), _stream())
    return False

  # the riders of the fused tail (er_emb_bwd_fused_tail); A/B switch
  tail_riders = os.environ.get('EASYREC_AMD_TAIL_RIDERS', '1') != '0'

  def dense_opt_fits_the_tail(self, wgrads, w, grad):
    """every queued weight gradient is a contiguous block of the flat gradient buffer (the optimizer finishes the k-split
    ones while it reads them), fp32 masters without bf16 shadows to refresh"""
    if self._bf16_state_of(w) is not None:
      return False
    lo, hi = grad.data_ptr(), grad.data_ptr() + 4 * grad.numel()
    return all(pr[2].is_contiguous() and lo <= pr[2].data_ptr() and pr[2].data_ptr() + 4 * pr[2].numel() <= hi for pr in wgrads)

  def _grad_groups(self, groups):
    arr = (GradGroup * len(groups))()
    keep = []
    for q, (dout, out, lam, has_base, terms) in zip(arr, groups):
      assert dout.shape == out.shape and dout.stride() == out.stride() and dout.stride(1) == 1 and len(terms) <= 4
      q.dout, q.out, q.ld = dout.data_ptr(), out.data_ptr(), dout.stride(0)
      q.batch, q.width, q.has_base, q.n_terms, q.lam = dout.shape[0], dout.shape[1], int(bool(has_base)), len(terms), lam
      for t, term in zip(q.terms, terms):
        g = term[1]
        assert g.dtype == torch.float32 and (g.dim() == 1 or g.stride(-1) == 1)
        t.g, t.g_ld = g.data_ptr(), (g.stride(0) if g.dim() >= 1 else 1)
        if term[0] == 'rowsum':
          t.kind, t.col0, t.width, t.dim = GRAD_TERM_ROWSUM, term[2], term[3], 1
        else:
          saved = _f32c(term[2])
          keep.append(saved)
          t.kind, t.col0, t.width, t.dim, t.saved = GRAD_TERM_FM, term[3], term[4], term[5], saved.data_ptr()
    return arr, keep

  def axpy2d(self, x, alpha, y, accumulate=True):
    """y (+)= alpha * x on 2-D views with unit inner stride."""
    rows, cols = x.shape
    assert x.stride(1) == 1 and y.stride(1) == 1 and y.shape == x.shape
    self.ck.er_axpy2d(_p(x), x.stride(0), alpha, _p(y), y.stride(0), rows, cols,
                      int(accumulate), _stream())

  # -- K6 / K7 cross
  def cross_v1_fwd(self, x0, w, b):
    B, d = x0.shape
    L = w.shape[0]
    out = torch.empty_like(x0)
    dots = torch.empty(B, L, dtype=torch.float32, device=x0.device)
    self.ck.er_cross_v1_fwd(_p(_f32c(x0)), _p(_f32c(w)), _p(_f32c(b)), B, d, L, _p(out), _p(dots),
                            _stream())
    return out, dots

  def cross_v1_bwd(self, x0, w, b, dots, dout):
    B, d = x0.shape
    L = w.shape[0]
    npart = self.lib.er_cross_v1_bwd_partials(B)
    dx0 = torch.empty_like(x0)
    dwp = torch.empty(npart, L * d, dtype=torch.float32, device=x0.device)
    dbp = torch.empty(npart, L * d, dtype=torch.float32, device=x0.device)
    self.ck.er_cross_v1_bwd(_p(x0), _p(w), _p(b), _p(dots), _p(_f32c(dout)), B, d, L, _p(dx0), _p(dwp),
                            _p(dbp), _stream())
    dw = self.colsum(dwp).view(L, d)
    db = self.colsum(dbp).view(L, d)
    return dx0, dw, db

  def cross_v2_fwd(self, x0, x, u, bias, diag_scale):
    B, d = x0.shape
    out = torch.empty_like(x0)
    self.ck.er_cross_v2_epilogue_fwd(_p(_f32c(x0)), _p(_f32c(x)), _p(_f32c(u)), _p(bias),
                                     diag_scale, B, d, _p(out), _stream())
    return out

  def cross_v2_bwd(self, x0, x, u, bias, diag_scale, dout):
    B, d = x0.shape
    dx0, dx, du = torch.empty_like(x0), torch.empty_like(x0), torch.empty_like(x0)
    self.ck.er_cross_v2_epilogue_bwd(_p(x0), _p(x), _p(u), _p(bias), diag_scale,
                                     _p(_f32c(dout)), B, d, _p(dx0), 0, _p(dx), _p(du), _stream())
    return dx0, dx, du

  # The DCN-v2 cross layer as ONE launch forward and one or two backward (north_star: "DCN-cross ... as fused HIP kernels";
  # reference layers/keras/interaction.py:249-286): the elementwise part rides in the epilogue of the layer's contraction
  # (er_gemm_f32_cross / er_gemm_bf16_nt_epi).  A/B switch: '0' = GEMM + er_cross_v2_epilogue_* launches.
  fused_cross = os.environ.get('EASYREC_AMD_FUSED_CROSS', '1') != '0'

  def _cross_b16(self, w, bf16, *rows):
    """The Bf16Shadows a bf16 cross contraction over weight w runs on (None: the fp32 kernel), or False: bf16 was asked
    for but er_gemm_bf16_nt_epi does not take these operands (the caller uses the unfused launches)."""
    if not bf16:
      return None
    st = self._bf16_state_of(w) if (self.bf16_nt and self.bf16_epilogues) else None
    if st is None or w.shape[0] % 4 or w.shape[1] % 4 or not self._nt_rows_ok(*rows):
      return False
    return st

  def cross_fwd_fused(self, x0, x, w, bias, diag, bf16):
    """(out, u) = (x0 * (x . w + bias + diag * x) + x, x . w) in one launch; None: not applicable."""
    B, d = x.shape
    if w.shape != (d, d) or x0.shape != x.shape or x0.stride(1) != 1 or x.stride(1) != 1:
      return None
    out = torch.empty(B, d, dtype=torch.float32, device=x.device)
    u = torch.empty(B, d, dtype=torch.float32, device=x.device)
    st = self._cross_b16(w, bf16, x0, x, out, u)
    if st is False:
      return None
    epi = GemmEpilogue(kind=EPI_CROSS_FWD, diag=float(diag), x0=x0.data_ptr(), xl=x.data_ptr(), u=u.data_ptr(),
                       ld_x0=x0.stride(0), ld_xl=x.stride(0), ld_u=u.stride(0))
    if st is not None:
      _, plain, t = st.weight(w)
      self.gemm_bf16_nt(st.act(x, cache=True), t, B, d, d, out=out, out_bf16=st.new_copy(out), bias=bias, epi=epi)
    else:
      self._log_gemm('gemm_f32_cross_kernel<true, false, 3>', None, B, d, d)
      self.ck.er_gemm_f32_cross(GEMM_NN, B, d, d, _p(x), x.stride(0), _p(w),
                                w.stride(0), _p(out), out.stride(0), _p(bias), 0,
                                ctypes.byref(epi), _stream())
    return out, u

  def cross_bwd_top(self, x0, x, u, bias, diag, dout, dx0, acc0, bf16, w):
    """The elementwise backward of a cross layer whose dout comes from outside the stack: du = dout * x0 (and its bf16 copy
    in a bf16 step), dx0 (+)= dout * (u + bias + diag * x), partial [row tiles, d] = per-tile column sums of du."""
    B, d = x0.shape
    du = torch.empty(B, d, dtype=torch.float32, device=x0.device)
    partial = torch.empty(self.gemm_row_tiles(B), d, dtype=torch.float32, device=x0.device)
    st = self._cross_b16(w, bf16, du) if bf16 else None
    dub = None
    if st:
      dub = torch.empty(B, st.pad8(d), dtype=torch.bfloat16, device=x0.device)  # (the kernel zeroes the k-tail columns)
      st.register(du, dub)
    self.ck.er_cross_v2_bwd_top(_p(x0), _p(x), _p(u), _p(bias), diag, _p(dout), dout.stride(0), B, d, _p(dx0),
                                dx0.stride(0), acc0, _p(du), _p(dub), 0 if dub is None else dub.stride(0),
                                _p(partial), _stream())
    return du, partial

  def cross_dgrad_fused(self, du, w, dout, diag, bf16, dst, acc, prev=None):
    """dst (+)= du . w^T + dout + diag * du - the whole gradient of the layer's input x_{l-1} - in one launch; with prev =
    dict(x0, u, bias, xl, dx0, acc0) (x_{l-1} is the output of the cross layer below) the same launch runs that layer's
    elementwise backward on it: returns (du_prev, partial_prev) (its du = dst * x0 and the per-tile column sums), else
    (None, None).  False: not applicable (bf16 operands the epilogue does not take)."""
    B, d = du.shape
    st = self._cross_b16(w, bf16, du, dout, dst, *( [prev['x0'], prev['u'], prev['dx0']] if prev else []))
    if st is False:
      return False
    epi = GemmEpilogue(kind=EPI_CROSS_BWD, diag=float(diag), dout=dout.data_ptr(), ld_dout=dout.stride(0))
    if diag != 0:
      epi.du_in, epi.ld_du_in = du.data_ptr(), du.stride(0)
    du_prev = partial = None
    if prev is not None:
      du_prev = torch.empty(B, d, dtype=torch.float32, device=du.device)
      partial = torch.empty(self.gemm_row_tiles(B), d, dtype=torch.float32, device=du.device)
      epi.x0, epi.ld_x0 = prev['x0'].data_ptr(), prev['x0'].stride(0)
      epi.prev_u, epi.ld_prev_u = prev['u'].data_ptr(), prev['u'].stride(0)
      epi.prev_bias = _p(prev['bias'])
      if diag != 0:
        epi.xl, epi.ld_xl = prev['xl'].data_ptr(), prev['xl'].stride(0)
      epi.dx0, epi.ld_dx0, epi.accumulate_dx0 = prev['dx0'].data_ptr(), prev['dx0'].stride(0), int(bool(prev['acc0']))
      epi.du_out, epi.ld_du_out = du_prev.data_ptr(), du_prev.stride(0)
      epi.partial = partial.data_ptr()
      if st is not None:
        dpb = st.new_copy(du_prev)
        epi.du_out_bf16, epi.ld_du_out_bf16 = dpb.data_ptr(), dpb.stride(0)
    if st is not None:
      _, plain, t = st.weight(w)
      self.gemm_bf16_nt(st.act(du), plain, B, d, d, out=dst, accumulate=acc, epi=epi)
    else:
      self._log_gemm('gemm_f32_cross_kernel<true, true, 4>', None, B, d, d)
      self.ck.er_gemm_f32_cross(GEMM_NT, B, d, d, _p(du), du.stride(0), _p(w), w.stride(0), _p(dst),
                                dst.stride(0), None, acc, ctypes.byref(epi), _stream())
    return du_prev, partial

  def cross_v2_bwd_acc(self, x0, x, u, bias, diag_scale, dout, dx0, acc0, dx, accx):
    """er_cross_v2_epilogue_bwd_acc: dx0 / dx are 2-D destinations (unit inner stride; dx None: x is x0) written or, with
    their flag, accumulated into.  Returns du."""
    B, d = x0.shape
    du = torch.empty_like(x0)
    assert dx0.stride(1) == 1 and (dx is None or dx.stride(1) == 1)
    assert dout.dim() == 2 and dout.stride(1) == 1 and dout.dtype == torch.float32
    self.ck.er_cross_v2_epilogue_bwd_acc(_p(x0), _p(x), _p(u), _p(bias), diag_scale, _p(dout),
                                         dout.stride(0), B, d, _p(dx0), dx0.stride(0), acc0, _p(dx),
                                         dx.stride(0) if dx is not None else 0, accx,
                                         _p(du), _stream())
    return du

  # -- K8 DIN
  def din_concat_fwd(self, q, h):
    B, L, E = h.shape
    out = torch.empty(B, L, 4 * E, dtype=torch.float32, device=h.device)
    self.ck.er_din_concat_fwd(_p(_f32c(q)), _p(_f32c(h)), B, L, E, _p(out), _stream())
    return out

  def din_concat_bwd(self, q, h, dout, dh=None, acc_h=False):
    """dh given: the history's gradient buffer of the step (kernels.grad_slot); acc_h: add into it."""
    B, L, E = h.shape
    dq = torch.empty_like(q)
    if dh is None:
      assert not acc_h
      dh = torch.empty_like(h)
    assert dh.shape == h.shape and dh.is_contiguous()
    self.ck.er_din_concat_bwd(_p(q), _p(h), _p(_f32c(dout)), B, L, E, _p(dq), 0, _p(dh), acc_h, _stream())
    return dq, dh

  # DIN's first attention layer on the GENERATED [q, h, q - h, q * h] operand (er_din_gemm_*): the [B, L, 4E] block exists
  # neither forward nor backward.  A/B switch: '0' = er_din_concat + the ordinary contractions.
  din_fused = os.environ.get('EASYREC_AMD_DIN_FUSED', '1') != '0'

  @staticmethod
  def din_gemm_ok(q, h, w):
    """q [B, E], h [B, L, E] contiguous fp32, w [4E, N]: shapes er_din_gemm_* take (E % 16 == 0, 16-byte aligned rows)."""
    if h.dim() != 3 or q.dim() != 2:
      return False
    B, L, E = h.shape
    return (E % 16 == 0 and L >= 2 and q.shape == (B, E) and q.is_contiguous() and h.is_contiguous() and w.shape[0] == 4 * E and
            w.stride(1) == 1 and w.stride(0) % 4 == 0 and q.data_ptr() % 16 == 0 and h.data_ptr() % 16 == 0 and
            w.data_ptr() % 16 == 0 and B * L * L < 2 ** 32)

  def din_gemm_fwd(self, q, h, w, bias, col_stats=None):
    """z [B * L, N] = [q, h, q - h, q * h] . w (+ bias) without building the block; col_stats as gemm()'s."""
    B, L, E = h.shape
    N = w.shape[1]
    z = torch.empty(B * L, N, dtype=torch.float32, device=h.device)
    self._log_gemm('gemm_f32_din_kernel<true, false, 1>', None, B * L, N, 4 * E)
    self.ck.er_din_gemm_fwd(_p(q), q.stride(0), _p(h), E, B, L, E, _p(w), w.stride(0), N, _p(bias), _p(z), N,
                            _p(col_stats), _stream())
    return z

  def din_gemm_wgrad(self, q, h, dz, out, accumulate=True):
    """out [4E, N] (+)= [q, h, q - h, q * h]^T . dz"""
    B, L, E = h.shape
    N = dz.shape[1]
    assert dz.shape[0] == B * L and dz.stride(1) == 1 and out.shape == (4 * E, N) and out.stride(1) == 1
    self._log_gemm('gemm_f32_din_kernel<false, false, 1>', None, 4 * E, N, B * L)
    self.ck.er_din_gemm_wgrad(_p(q), q.stride(0), _p(h), E, B, L, E, _p(dz), dz.stride(0), N, _p(out),
                              out.stride(0), accumulate, _stream())
    return out

  def din_gemm_dgrad(self, dz, w, q, h, dh=None, acc_h=False):
    """(dq [B, E], dh [B, L, E]) from dz [B * L, N] and w [4E, N] without building dcat = dz . w^T; dh given: the history's
    gradient buffer of the step (kernels.grad_slot), acc_h: add into it."""
    B, L, E = h.shape
    N = dz.shape[1]
    dq = torch.empty(B, E, dtype=torch.float32, device=h.device)
    if dh is None:
      assert not acc_h
      dh = torch.empty_like(h)
    assert dh.shape == h.shape and dh.is_contiguous()
    n_part = int(self.lib.er_din_dq_partial_floats(B, L, E))
    partial = torch.empty(n_part, dtype=torch.float32, device=h.device)
    self._log_gemm('gemm_f32_din_kernel<true, true, 2>', None, B * L, 4 * E, N)
    self.ck.er_din_gemm_dgrad(_p(dz), dz.stride(0), N, _p(w), w.stride(0), _p(q), q.stride(0), _p(h), E, B, L,
                              E, _p(dq), E, _p(dh), E, acc_h, _p(partial), _stream())
    return dq, dh

  def din_pool_fwd(self, scores, hist, seq_len, scale=1.0):
    B, L, E = hist.shape
    probs = torch.empty(B, L, dtype=torch.float32, device=hist.device)
    out = torch.empty(B, E, dtype=torch.float32, device=hist.device)
    self.ck.er_din_pool_fwd(_p(_f32c(scores)), _p(_f32c(hist)), _p(seq_len), B, L, E, scale,
                            _p(probs), _p(out), _stream())
    return out, probs

  def din_pool_bwd(self, probs, hist, seq_len, dout, scale=1.0, dhist=None, acc_h=False):
    B, L, E = hist.shape
    dscores = torch.empty(B, L, dtype=torch.float32, device=hist.device)
    if dhist is None:
      assert not acc_h
      dhist = torch.empty_like(hist)
    assert dhist.shape == hist.shape and dhist.is_contiguous()
    self.ck.er_din_pool_bwd(_p(probs), _p(hist), _p(seq_len), _p(_f32c(dout)), B, L, E,
                            scale, _p(dscores), _p(dhist), acc_h, _stream())
    return dscores, dhist

  # -- K8e the gradient reduce of the blocks with packed parameters (K8b, K8d)
  def theta_grad_reduce(self, partials, rows, grads, row_groups, acc):
    """`grads` (a ThetaGradTable) (+)= the sum over the rows of partials [rows, P]; row_groups (1 or 8) is the
    summation order easyrec_hip.h states."""
    self.ck.er_theta_grad_reduce(_p(partials), rows, partials.numel() // rows, grads.lens, len(grads.grads),
                                 grads.table, row_groups, bool(acc), _stream())

  # -- K8b BST transformer block (model/multi_tower_bst.py)
  BST_MAX_T = 64
  BST_MAX_E = 64

  def bst_param_count(self, E, H):
    return int(self.lib.er_bst_param_count(int(E), int(H)))

  def bst_grid(self, B):
    return int(self.lib.er_bst_grid(int(B)))

  def _bst_flops(self, B, T, E, H):
    # per example: Q / K / V (2 T sum p_h^2 each), S and P V (2 T^2 E each), the two E x E projections (2 T E^2 each)
    p = -(-E // H)
    nh = -(-E // p)
    last = E - (nh - 1) * p
    qkv = 3 * 2.0 * T * ((nh - 1) * p * p + last * last)
    return B * (qkv + 4.0 * T * T * E + 4.0 * T * E * E)

  def bst_fwd(self, key, hist, seq_len, theta, T, H):
    """key [B, E], hist [B, L, E] (the lookup's static buffer), seq_len [B] int32, theta: the packed parameters
    (er_bst_param_count).  Returns [B, T * E]."""
    B, L, E = hist.shape
    assert key.shape == (B, E) and seq_len.dtype == torch.int32
    out = torch.empty(B, T * E, dtype=torch.float32, device=hist.device)
    self.ck.er_bst_fwd(_p(_f32c(key)), _p(_f32c(hist)), _p(seq_len), _p(_f32c(theta)), B, L, T,
                       E, H, _p(out), _stream())
    if self.op_log is not None:
      self.op_log.append(('er::bst_fwd_kernel', self._bst_flops(B, T, E, H)))
    return out

  def bst_bwd(self, key, hist, seq_len, theta, dout, T, H, grads, dhist=None, acc_h=False):
    """dkey [B, E] and dhist [B, L, E] (written, or added into with acc_h); the parameter gradients are ADDED into
    `grads` (a ThetaGradTable: the variables' gradient buffers in theta's order)."""
    B, L, E = hist.shape
    dkey = torch.empty(B, E, dtype=torch.float32, device=hist.device)
    if dhist is None:
      assert not acc_h
      dhist = torch.empty_like(hist)
    assert dhist.shape == hist.shape and dhist.is_contiguous()
    rows = self.bst_grid(B)
    partials = torch.empty(rows * self.bst_param_count(E, H), dtype=torch.float32, device=hist.device)
    self.ck.er_bst_bwd(_p(_f32c(key)), _p(_f32c(hist)), _p(seq_len), _p(_f32c(theta)), _p(_f32c(dout)), B, L,
                       T, E, H, _p(dkey), _p(dhist), acc_h, _p(partials), _stream())
    self.theta_grad_reduce(partials, rows, grads, 1, True)
    if self.op_log is not None:
      self.op_log.append(('er::bst_bwd_kernel', 2.0 * self._bst_flops(B, T, E, H)))
    return dkey, dhist

  # -- K8c AutoInt self-attention core (layers/multihead_attention.py)
  AUTOINT_LDS_BUDGET = 65536  # bytes per workgroup (csrc/er_autoint.hip)

  def autoint_lds_bytes(self, F, H, ds):
    return int(self.lib.er_autoint_lds_bytes(int(F), int(H), int(ds)))

  def autoint_epb(self, F, H, ds, bwd):
    return int(self.lib.er_autoint_epb(int(F), int(H), int(ds), bwd))

  def autoint_pack(self, wq, wk, wv, wr):
    """[wq | wk | wv | wr] ([din, d] each) -> [din, 4d]: one launch."""
    din, d = wq.shape
    assert all(w.shape == (din, d) for w in (wk, wv, wr))
    out = torch.empty(din, 4 * d, dtype=torch.float32, device=wq.device)
    self.ck.er_autoint_pack(_p(_f32c(wq)), _p(_f32c(wk)), _p(_f32c(wv)), _p(_f32c(wr)), din, d, _p(out),
                            _stream())
    return out

  def autoint_attn_fwd(self, qkvr, F, H, ds):
    """qkvr [B * F, 4d] (Q | K | V | R per field row) -> y = relu(softmax(Q_h K_h^T sqrt(ds)) V_h + R) [B * F, d]."""
    rows, w = qkvr.shape
    d = H * ds
    assert w == 4 * d and rows % F == 0
    B = rows // F
    y = torch.empty(rows, d, dtype=torch.float32, device=qkvr.device)
    self.ck.er_autoint_attn_fwd(_p(_f32c(qkvr)), B, F, H, ds, _p(y), _stream())
    if self.op_log is not None:
      self.op_log.append(('er::autoint_attn_fwd_kernel', 4.0 * B * F * F * d))
    return y

  def autoint_attn_bwd(self, qkvr, y, dy, F, H, ds):
    """-> dqkvr [B * F, 4d] = dQ | dK | dV | dR (easyrec_hip.h K8c)."""
    rows, w = qkvr.shape
    B = rows // F
    assert y.shape == dy.shape == (rows, H * ds)
    dq = torch.empty_like(qkvr)
    self.ck.er_autoint_attn_bwd(_p(_f32c(qkvr)), _p(_f32c(y)), _p(_f32c(dy)), B, F, H, ds,
                                _p(dq), _stream())
    if self.op_log is not None:
      self.op_log.append(('er::autoint_attn_bwd_kernel', 12.0 * B * F * F * H * ds))
    return dq

  # -- K8f BERT-style encoder pieces (layers/multihead_cross_attention.py)
  MHA_LDS_BUDGET = 81920  # bytes per workgroup (csrc/er_mha.hip)
  MHA_MAX_DS = 128
  ADD_LN_MAX_W = 4096

  def mha_lds_bytes(self, F, T, ds, bwd=True):
    return int(self.lib.er_mha_lds_bytes(int(F), int(T), int(ds), bool(bwd)))

  def mha_pack(self, ws, bs):
    """[w_0 | w_1 (| w_2)] ([din, d] each) -> [din, n d] and the biases side by side [n d]: one launch."""
    n = len(ws)
    din, d = ws[0].shape
    assert n in (2, 3) and len(bs) == n and all(w.shape == (din, d) for w in ws) and all(b.shape == (d,) for b in bs)
    w = torch.empty(din, n * d, dtype=torch.float32, device=ws[0].device)
    bias = torch.empty(n * d, dtype=torch.float32, device=ws[0].device)
    ws = [_f32c(t) for t in ws] + [None] * (3 - n)
    bs = [_f32c(t) for t in bs] + [None] * (3 - n)
    self.ck.er_mha_pack(_p(ws[0]), _p(ws[1]), _p(ws[2]), _p(bs[0]), _p(bs[1]), _p(bs[2]), n, din, d, _p(w), _p(bias),
                        _stream())
    return w, bias

  @staticmethod
  def _mha_operand(t, rows, d, what):
    assert t.dim() == 2 and t.shape == (rows, d) and t.stride(1) == 1 and t.stride(0) >= d and \
        t.dtype == torch.float32, '%s: [%d, %d] fp32 rows with unit inner stride expected' % (what, rows, d)
    return t

  def _mha_fwd(self, group, q, k, v, to_mask, B, F, T, H, ds):
    """mha_fwd (group False) | mha_group_fwd (True): the checks, the launch and the op-log line of both."""
    name, entry = ('mha_group_fwd', self.ck.er_mha_group_fwd) if group else ('mha_fwd', self.ck.er_mha_fwd)
    d = H * ds
    self._mha_operand(q, B * F, d, name + ' q')
    self._mha_operand(k, B * T, d, name + ' k')
    self._mha_operand(v, B * T, d, name + ' v')
    assert to_mask is None or (to_mask.dtype == torch.int32 and to_mask.shape == (B, T) and to_mask.is_contiguous())
    ctx = torch.empty(B * F, d, dtype=torch.float32, device=q.device)
    entry(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(to_mask), B, F, T, H, ds, _p(ctx), _stream())
    if self.op_log is not None:
      self.op_log.append(('er::%s_kernel' % name, 4.0 * B * F * T * d))
    return ctx

  def _mha_bwd(self, group, q, k, v, to_mask, dctx, B, F, T, H, ds, dq, dk, dv):
    """mha_bwd (group False) | mha_group_bwd (True)."""
    name, entry = ('mha_group_bwd', self.ck.er_mha_group_bwd) if group else ('mha_bwd', self.ck.er_mha_bwd)
    d = H * ds
    self._mha_operand(q, B * F, d, name + ' q')
    self._mha_operand(k, B * T, d, name + ' k')
    self._mha_operand(v, B * T, d, name + ' v')
    self._mha_operand(dq, B * F, d, name + ' dq')
    self._mha_operand(dk, B * T, d, name + ' dk')
    self._mha_operand(dv, B * T, d, name + ' dv')
    assert dctx.shape == (B * F, d)
    assert to_mask is None or (to_mask.dtype == torch.int32 and to_mask.shape == (B, T) and to_mask.is_contiguous())
    entry(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(to_mask), _p(_f32c(dctx)), B, F, T, H, ds,
          _p(dq), dq.stride(0), _p(dk), dk.stride(0), _p(dv), dv.stride(0), _stream())
    if self.op_log is not None:
      self.op_log.append(('er::%s_kernel' % name, 12.0 * B * F * T * d))

  def mha_fwd(self, q, k, v, to_mask, B, F, T, H, ds):
    """q [B * F, H ds], k, v [B * T, H ds]: 2-D fp32 views with unit inner stride (column blocks of a packed buffer or
    tensors of their own), to_mask int32 [B, T] or None -> ctx [B * F, H ds] = concat_h softmax(Q_h K_h^T / sqrt(ds)
    + adder) V_h."""
    return self._mha_fwd(False, q, k, v, to_mask, B, F, T, H, ds)

  def mha_bwd(self, q, k, v, to_mask, dctx, B, F, T, H, ds, dq, dk, dv):
    """dq [B * F, H ds], dk, dv [B * T, H ds] (views as above, written) from dctx [B * F, H ds] (contiguous)."""
    self._mha_bwd(False, q, k, v, to_mask, dctx, B, F, T, H, ds, dq, dk, dv)

  def mha_group_units(self, F, T, ds):
    """Units per workgroup of the grouped attention launches: 8, 4 or 2; 1: only one fits; 0: outside the envelope."""
    return int(self.lib.er_mha_group_units(int(F), int(T), int(ds)))

  def mha_group_fwd(self, q, k, v, to_mask, B, F, T, H, ds):
    """mha_fwd's arguments and result bits, several (example, head) units per workgroup (mha_group_units >= 2)."""
    return self._mha_fwd(True, q, k, v, to_mask, B, F, T, H, ds)

  def mha_group_bwd(self, q, k, v, to_mask, dctx, B, F, T, H, ds, dq, dk, dv):
    """mha_bwd's arguments and result bits, several units per workgroup."""
    self._mha_bwd(True, q, k, v, to_mask, dctx, B, F, T, H, ds, dq, dk, dv)

  SEGMENT_MEAN_MAX_W = 4096
  SEGMENT_MEAN_MAX_S = 4096
  SEGMENT_MEAN_MAX_SEG = 64

  @staticmethod
  def _segment_mean_operands(seg_begin, lens, B, n_seg):
    assert seg_begin.dtype == torch.int32 and seg_begin.shape == (n_seg + 1,) and seg_begin.is_contiguous()
    assert lens is None or (lens.dtype == torch.int32 and lens.shape == (B, n_seg) and lens.is_contiguous())

  def segment_mean_fwd(self, x, seg_begin, lens, n_seg):
    """x [B, S, W], seg_begin int32 [n_seg + 1] on the device (0 .. S ascending), lens int32 [B, n_seg] or None ->
    out [B, n_seg, W]: per segment the mean of its first len rows (len == 0: NaN)."""
    B, S, W = x.shape
    self._segment_mean_operands(seg_begin, lens, B, n_seg)
    out = torch.empty(B, n_seg, W, dtype=torch.float32, device=x.device)
    self.ck.er_segment_mean_fwd(_p(_f32c(x)), _p(seg_begin), _p(lens), B, S, W, n_seg, _p(out), _stream())
    if self.op_log is not None:
      self.op_log.append(('er::segment_mean_fwd_kernel', 1.0 * B * S * W))
    return out

  def segment_mean_bwd(self, dout, seg_begin, lens, S):
    """dout [B, n_seg, W] -> dx [B, S, W] (every element written): dout / len on a segment's first len rows, else 0."""
    B, n_seg, W = dout.shape
    self._segment_mean_operands(seg_begin, lens, B, n_seg)
    dx = torch.empty(B, S, W, dtype=torch.float32, device=dout.device)
    self.ck.er_segment_mean_bwd(_p(_f32c(dout)), _p(seg_begin), _p(lens), B, S, W, n_seg, _p(dx), _stream())
    if self.op_log is not None:
      self.op_log.append(('er::segment_mean_bwd_kernel', 1.0 * B * S * W))
    return dx

  def add_ln_grid(self, rows, W):
    return int(self.lib.er_add_ln_grid(int(rows), int(W)))

  def add_ln_fwd(self, x, res, gamma, beta, eps):
    """x [rows, W], res [res_rows, W] (read at row % res_rows) or None -> (y, mean [rows], rstd [rows])."""
    rows, W = x.shape
    assert res is None or (res.dim() == 2 and res.shape[1] == W and rows % res.shape[0] == 0)
    assert gamma.shape == (W,) and beta.shape == (W,)
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    self.ck.er_add_ln_fwd(_p(_f32c(x)), _p(None if res is None else _f32c(res)), rows,
                          1 if res is None else res.shape[0], W, _p(_f32c(gamma)), _p(_f32c(beta)), float(eps), _p(y),
                          _p(mean), _p(rstd), _stream())
    if self.op_log is not None:
      self.op_log.append(('er::add_ln_fwd_kernel', 8.0 * rows * W))
    return y, mean, rstd

  def add_ln_bwd(self, dy, x, res, gamma, mean, rstd, grads, acc):
    """-> dz [rows, W], the gradient with respect to x + res; dgamma and dbeta are added into (acc) or written to
    `grads` (a ThetaGradTable of gamma's and beta's buffers) by the shared fixed-order reduce."""
    rows, W = x.shape
    assert dy.shape == x.shape and mean.numel() == rows and rstd.numel() == rows
    dz = torch.empty_like(x)
    grid = self.add_ln_grid(rows, W)
    partials = torch.empty(grid * 2 * W, dtype=torch.float32, device=x.device)
    self.ck.er_add_ln_bwd(_p(_f32c(dy)), _p(_f32c(x)), _p(None if res is None else _f32c(res)), rows,
                          1 if res is None else res.shape[0], W, _p(_f32c(gamma)), _p(mean), _p(rstd), _p(dz),
                          _p(partials), _stream())
    self.theta_grad_reduce(partials, grid, grads, 8, acc)
    if self.op_log is not None:
      self.op_log.append(('er::add_ln_bwd_kernel', 12.0 * rows * W))
    return dz

  # -- K8i MaskNet's mask multiply and LayerNorm + ReLU (layers/keras/mask_net.py)
  @staticmethod
  def _rows_table(ts, what):
    """HOST arrays of the addresses and row pitches of 2-D fp32 tensors whose rows are contiguous (column slices of a
    wider tensor included)."""
    for t in ts:
      assert t.dim() == 2 and t.dtype == torch.float32 and (t.shape[1] == 1 or t.stride(1) == 1), what
    return ((ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts]),
            (ctypes.c_int64 * len(ts))(*[t.stride(0) if t.shape[0] > 1 else t.shape[1] for t in ts]))

  @staticmethod
  def _row_major(t):
    return t if (t.dim() == 2 and (t.shape[1] == 1 or t.stride(1) == 1) and (t.shape[0] == 1 or t.stride(0) >= t.shape[1])) \
        else t.contiguous()

  def mask_mul_fwd(self, x, vs):
    """x [B, W], vs: n tensors [B, W] (row pitches of their own) -> n fresh tensors x * v_i, one launch."""
    B, W = x.shape
    x, vs = self._row_major(x), [self._row_major(v) for v in vs]
    assert all(v.shape == (B, W) for v in vs)
    outs = [torch.empty(B, W, dtype=torch.float32, device=x.device) for _ in vs]
    (xp, ldx), (vp, ldv), (op, ldo) = self._rows_table([x], 'x'), self._rows_table(vs, 'v'), self._rows_table(outs, 'out')
    self.ck.er_mask_mul_fwd(xp[0], ldx[0], vp, ldv, len(vs), B, W, op, ldo, _stream())
    if self.op_log is not None:
      self.op_log.append(('er::mask_mul_fwd_kernel', 1.0 * len(vs) * B * W))
    return outs

  def mask_mul_bwd(self, x, vs, douts, want_dx=True):
    """-> ([dv_i = dout_i * x], dx = sum_i dout_i * v_i or None), one launch."""
    B, W = x.shape
    x, vs = self._row_major(x), [self._row_major(v) for v in vs]
    douts = [self._row_major(d) for d in douts]
    assert len(douts) == len(vs) and all(t.shape == (B, W) for t in vs + douts)
    dvs = [torch.empty(B, W, dtype=torch.float32, device=x.device) for _ in vs]
    dx = torch.empty(B, W, dtype=torch.float32, device=x.device) if want_dx else None
    (xp, ldx), (vp, ldv) = self._rows_table([x], 'x'), self._rows_table(vs, 'v')
    (dp, ldd), (op, ldo) = self._rows_table(douts, 'dout'), self._rows_table(dvs, 'dv')
    self.ck.er_mask_mul_bwd(xp[0], ldx[0], vp, ldv, dp, ldd, len(vs), B, W, op, ldo, _p(dx), W, _stream())
    if self.op_log is not None:
      self.op_log.append(('er::mask_mul_bwd_kernel', (3.0 if want_dx else 1.0) * len(vs) * B * W))
    return dvs, dx

  def ln_relu_grid(self, B, O, n):
    return int(self.lib.er_ln_relu_grid(int(B), int(O), int(n)))

  def ln_relu_fwd(self, hs, gammas, betas, eps, y=None):
    """hs: n tensors [B, O]; gammas, betas: n tensors [O] -> (y [B, n * O], mean [n, B], rstd [n, B]); y: the [B, n * O]
    column block of a wider row-major buffer to write into (fresh when None)."""
    n, (B, O) = len(hs), hs[0].shape
    hs = [self._row_major(h) for h in hs]
    assert all(h.shape == (B, O) for h in hs) and all(t.shape == (O,) and t.is_contiguous() for t in gammas + betas)
    if y is None:
      y = torch.empty(B, n * O, dtype=torch.float32, device=hs[0].device)
    assert y.shape == (B, n * O) and y.dtype == torch.float32
    mean = torch.empty(n, B, dtype=torch.float32, device=y.device)
    rstd = torch.empty(n, B, dtype=torch.float32, device=y.device)
    (hp, ldh), (yp, ldy) = self._rows_table(hs, 'h'), self._rows_table([y], 'y')
    gp = (ctypes.c_void_p * n)(*[_p(_f32c(g)) for g in gammas])
    bp = (ctypes.c_void_p * n)(*[_p(_f32c(b)) for b in betas])
    self.ck.er_ln_relu_fwd(hp, ldh, gp, bp, n, B, O, float(eps), yp[0], ldy[0], _p(mean), _p(rstd), _stream())
    if self.op_log is not None:
      self.op_log.append(('er::ln_relu_fwd_kernel', 9.0 * n * B * O))
    return y, mean, rstd

  def ln_relu_bwd(self, dy, y, hs, gammas, mean, rstd, grads, acc):
    """dy, y [B, n * O] (row pitches of their own) -> [dh_i [B, O]]; dgamma_i and dbeta_i are added into (acc) or written
    to `grads` (a ThetaGradTable in the order gamma_0, beta_0, gamma_1, ..) by the shared fixed-order reduce."""
    n, (B, O) = len(hs), hs[0].shape
    hs, dy, y = [self._row_major(h) for h in hs], self._row_major(dy), self._row_major(y)
    assert dy.shape == (B, n * O) and y.shape == (B, n * O) and len(grads.grads) == 2 * n
    dhs = [torch.empty(B, O, dtype=torch.float32, device=dy.device) for _ in hs]
    grid = self.ln_relu_grid(B, O, n)
    partials = torch.empty(grid * 2 * n * O, dtype=torch.float32, device=dy.device)
    (hp, ldh), (dp, ldd) = self._rows_table(hs, 'h'), self._rows_table(dhs, 'dh')
    (dyp, lddy), (yp, ldy) = self._rows_table([dy], 'dy'), self._rows_table([y], 'y')
    gp = (ctypes.c_void_p * n)(*[_p(_f32c(g)) for g in gammas])
    self.ck.er_ln_relu_bwd(dyp[0], lddy[0], yp[0], ldy[0], hp, ldh, gp, _p(mean), _p(rstd), n, B, O, dp, ldd,
                           _p(partials), _stream())
    self.theta_grad_reduce(partials, grid, grads, 8, acc)
    if self.op_log is not None:
      self.op_log.append(('er::ln_relu_bwd_kernel', 13.0 * n * B * O))
    return dhs

  # -- K8j PPNet's gate multiply (layers/keras/ppnet.py)
  def gate_scale_grid(self, B, W):
    return int(self.lib.er_gate_scale_grid(int(B), int(W)))

  def gate_scale_fwd(self, x, z, bias):
    """x, z [B, W] (row pitches of their own), bias [W] or None -> a fresh x * 2 * sigmoid(z + bias), one launch."""
    B, W = x.shape
    x, z = self._row_major(x), self._row_major(z)
    assert z.shape == (B, W) and (bias is None or (bias.shape == (W,) and bias.is_contiguous()))
    out = torch.empty(B, W, dtype=torch.float32, device=x.device)
    (p, ld) = self._rows_table([x, z, out], 'x, z, out')
    self.ck.er_gate_scale_fwd(p[0], ld[0], p[1], ld[1], _p(None if bias is None else _f32c(bias)), B, W, p[2], ld[2],
                              _stream())
    if self.op_log is not None:
      self.op_log.append(('er::gate_scale_fwd_kernel', 8.0 * B * W))
    return out

  def gate_scale_bwd(self, dout, x, z, bias, grads, acc, want_dx=True):
    """-> (dx = dout * g or None, dz = dout * x * g * (1 - g / 2)), g recomputed, one launch; with a bias its gradient
    (the column sums of dz) is added into (acc) or written to `grads` (a ThetaGradTable of the bias's buffer) by the
    shared fixed-order reduce."""
    B, W = x.shape
    dout, x, z = self._row_major(dout), self._row_major(x), self._row_major(z)
    assert dout.shape == (B, W) and z.shape == (B, W) and (bias is None or (grads is not None and len(grads.grads) == 1))
    dz = torch.empty(B, W, dtype=torch.float32, device=x.device)
    dx = torch.empty(B, W, dtype=torch.float32, device=x.device) if want_dx else None
    grid = self.gate_scale_grid(B, W)
    partials = torch.empty(grid * W, dtype=torch.float32, device=x.device) if bias is not None else None
    (p, ld) = self._rows_table([dout, x, z, dz], 'dout, x, z, dz')
    self.ck.er_gate_scale_bwd(p[0], ld[0], p[1], ld[1], p[2], ld[2], _p(None if bias is None else _f32c(bias)), B, W,
                              _p(dx), W, p[3], ld[3], _p(partials), _stream())
    if bias is not None:
      self.theta_grad_reduce(partials, grid, grads, 8, acc)
    if self.op_log is not None:
      self.op_log.append(('er::gate_scale_bwd_kernel', (12.0 if want_dx else 11.0) * B * W))
    return dx, dz

  # -- K8k variational dropout on a feature group's output (layers/variational_dropout_layer.py)
  def vdrop_grid(self, B, W):
    return int(self.lib.er_vdrop_grid(int(B), int(W)))

  @staticmethod
  def _vdrop_seg(seg):
    """seg: None (identity) or a VDropSeg -> (host array, device pointer)"""
    return (None, None) if seg is None else (seg.host, _p(seg.dev))

  def vdrop_fwd(self, x, logit_p, u, seg, lam):
    """x [B, W] (a row pitch of its own), logit_p [P], u [B, P] or None (evaluation), seg: a VDropSeg or None (identity, P
    == W), lam = lambda / B -> (a fresh x * m, penalty [1]), one launch."""
    B, W = x.shape
    P = logit_p.numel()
    x = self._row_major(x)
    u = None if u is None else self._row_major(u)
    assert (u is None or u.shape == (B, P)) and (seg is None or seg.W == W)
    out = torch.empty(B, W, dtype=torch.float32, device=x.device)
    penalty = torch.empty(1, dtype=torch.float32, device=x.device)
    (p, ld) = self._rows_table([x, out] + ([] if u is None else [u]), 'x, out, u')
    sh, sd = self._vdrop_seg(seg)
    self.ck.er_vdrop_fwd(p[0], ld[0], _p(_f32c(logit_p)), None if u is None else p[2], 0 if u is None else ld[2], sh, sd,
                         B, W, P, float(lam), p[1], ld[1], _p(penalty), _stream())
    if self.op_log is not None:
      self.op_log.append(('er::vdrop_fwd_kernel', 12.0 * B * W))
    return out, penalty

  def vdrop_bwd(self, dout, dpenalty, x, logit_p, u, seg, lam, grads, acc, want_dx=True):
    """-> dx = dout * m or None, m recomputed, one launch; dlogit_p (the batch sums and the penalty's own gradient times
    dpenalty [1], None for none) is added into (acc) or written to `grads` (a ThetaGradTable of logit_p's buffer) by the
    shared fixed-order reduce."""
    B, W = x.shape
    P = logit_p.numel()
    dout, x = self._row_major(dout), self._row_major(x)
    u = None if u is None else self._row_major(u)
    assert dout.shape == (B, W) and len(grads.grads) == 1 and (u is None or u.shape == (B, P))
    dx = torch.empty(B, W, dtype=torch.float32, device=x.device) if want_dx else None
    grid = self.vdrop_grid(B, W)
    partials = torch.empty((grid + 1) * P, dtype=torch.float32, device=x.device)
    (p, ld) = self._rows_table([dout, x] + ([] if u is None else [u]), 'dout, x, u')
    sh, sd = self._vdrop_seg(seg)
    self.ck.er_vdrop_bwd(p[0], ld[0], p[1], ld[1], _p(_f32c(logit_p)), None if u is None else p[2],
                         0 if u is None else ld[2], sh, sd, B, W, P, float(lam),
                         None if dpenalty is None else _p(_f32c(dpenalty)), _p(dx), W, _p(partials), _stream())
    self.theta_grad_reduce(partials, grid + 1, grads, 8, acc)
    if self.op_log is not None:
      self.op_log.append(('er::vdrop_bwd_kernel', (16.0 if want_dx else 15.0) * B * W))
    return dx

  # -- K8l multi-logit heads: softmax cross entropy and JRC (builders/multiclass_loss.py)
  def softmax_ce_grid(self, B, C):
    return int(self.lib.er_softmax_ce_grid(int(B), int(C)))

  def jrc_grid(self, B):
    return int(self.lib.er_jrc_grid(int(B)))

  def _softmax_ce_outputs(self, logits, labels, weights, want):
    assert logits.dim() == 2 and logits.dtype == torch.float32 and logits.stride(1) == 1
    B, C = logits.shape
    dev = logits.device
    y = None if labels is None else _f32c(labels)  # (None: a forward-only launch that reads no label)
    assert (y is None and not {'loss', 'dlogits', 'label_rank'} & set(want)) or y.numel() == B
    assert weights is None or _f32c(weights).numel() == B
    grid = self.softmax_ce_grid(B, C)
    assert grid > 0, 'er_softmax_ce: B = %d, C = %d outside the envelope' % (B, C)
    f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
    o = {}
    if 'loss' in want:
      o['loss_partials'] = f(grid)
      o['loss'] = f(1)
      o['loss']._er_partials = (o['loss_partials'], 1.0, 1.0)  # (the loss tail's launch sums them: scale 1, divisor 1)
    if 'dlogits' in want:
      o['dlogits'] = f(B, C)
    if 'probs' in want:
      o['probs'] = f(B, C)
    if 'y' in want:
      o['y'] = torch.empty(B, dtype=torch.int64, device=dev)
    if 'logits_y' in want:
      o['logits_y'] = f(B)
    if 'probs_y' in want:
      o['probs_y'] = f(B)
    if 'label_rank' in want:
      o['label_rank'] = torch.empty(B, dtype=torch.int32, device=dev)
    return y, o

  def softmax_ce(self, logits, labels, weights, loss_scale=1.0, want=('loss', 'dlogits', 'probs')):
    """er_softmax_ce: logits [B, C] (row stride >= C), labels [B] fp32 (None for a forward-only launch), weights [B] or
    None -> dict of the outputs named in `want` (loss, dlogits, probs, y, logits_y, probs_y, label_rank).  'loss': loss
    [1] with _er_partials set - the loss tail's launch sums loss_partials into it."""
    y, o = self._softmax_ce_outputs(logits, labels, weights, want)
    B, C = logits.shape
    self.ck.er_softmax_ce(logits.data_ptr(), logits.stride(0), _p(y), _p(weights), B, C, float(loss_scale),
                          _p(o.get('probs')), C, _p(o.get('y')), _p(o.get('logits_y')), _p(o.get('probs_y')),
                          _p(o.get('dlogits')), C, _p(o.get('label_rank')), _p(o.get('loss_partials')), _stream())
    return o

  def softmax_ce_multi(self, heads, want=('loss', 'dlogits', 'probs')):
    """heads: 1 to 8 of (logits, labels, weights or None, loss_scale) -> softmax_ce's dict per head, one launch
    (er_softmax_ce_multi: the training outputs loss, dlogits and probs only)."""
    assert set(want) <= {'loss', 'dlogits', 'probs'} and 1 <= len(heads) <= 8
    n = len(heads)
    vp, outs, keep = ctypes.c_void_p * n, [], []
    for logits, labels, weights, _ in heads:
      y, o = self._softmax_ce_outputs(logits, labels, weights, want)
      outs.append(o)
      keep.append(y)
    self.ck.er_softmax_ce_multi(
        n, vp(*[h[0].data_ptr() for h in heads]), (ctypes.c_int64 * n)(*[h[0].stride(0) for h in heads]),
        vp(*[y.data_ptr() for y in keep]), vp(*[_p(h[2]) for h in heads]),
        (ctypes.c_int64 * n)(*[h[0].shape[0] for h in heads]), (ctypes.c_int32 * n)(*[h[0].shape[1] for h in heads]),
        (ctypes.c_float * n)(*[float(h[3]) for h in heads]), vp(*[_p(o.get('probs')) for o in outs]),
        vp(*[_p(o.get('dlogits')) for o in outs]), vp(*[_p(o.get('loss_partials')) for o in outs]), _stream())
    return outs

  def jrc(self, logits, labels, session_keys, weights, alpha, ce_scale=1.0, loss_scale=1.0, want_grad=True):
    """er_jrc: logits [B, 2] (row stride >= 2), labels [B] fp32, session_keys [B] int64, weights [B] or None ->
    dict(loss [1] with _er_partials, loss_partials, dlogits [B, 2] or None, probs [B])."""
    assert logits.dim() == 2 and logits.shape[1] == 2 and logits.dtype == torch.float32 and logits.stride(1) == 1
    B = logits.shape[0]
    dev = logits.device
    assert session_keys.dtype == torch.int64 and session_keys.is_contiguous() and session_keys.numel() == B
    grid = self.jrc_grid(B)
    assert grid > 0, 'er_jrc: B = %d outside the envelope' % B
    o = {'loss_partials': torch.empty(grid, dtype=torch.float32, device=dev),
         'loss': torch.empty(1, dtype=torch.float32, device=dev),
         'dlogits': torch.empty(B, 2, dtype=torch.float32, device=dev) if want_grad else None,
         'probs': torch.empty(B, dtype=torch.float32, device=dev)}
    o['loss']._er_partials = (o['loss_partials'], 1.0, 1.0)
    self.ck.er_jrc(logits.data_ptr(), logits.stride(0), _p(_f32c(labels)), session_keys.data_ptr(),
                   None if weights is None else _p(_f32c(weights)), B, float(alpha), float(ce_scale), float(loss_scale),
                   _p(o['loss_partials']), _p(o['dlogits']), 2, _p(o['probs']), _stream())
    return o

  # -- K8d FiBiNet's field blocks (layers/keras/fibinet.py)
  def bilinear_lds_bytes(self, F, D):
    return int(self.lib.er_bilinear_lds_bytes(int(F), int(D)))

  def bilinear_epb(self, F, D, each):
    return int(self.lib.er_bilinear_epb(int(F), int(D), bool(each)))

  def bilinear_param_count(self, F, D, each):
    return int(self.lib.er_bilinear_param_count(int(F), int(D), bool(each)))

  def bilinear_fwd(self, x, theta, F, D, each, plus):
    """x [B, F * D], theta: the packed dense layers (er_bilinear_param_count) -> [B, F (F - 1) / 2] with plus,
    [B, F (F - 1) / 2 * D] without."""
    B = x.shape[0]
    assert x.shape == (B, F * D) and theta.numel() == self.bilinear_param_count(F, D, each)
    pairs = F * (F - 1) // 2
    out = torch.empty(B, pairs if plus else pairs * D, dtype=torch.float32, device=x.device)
    self.ck.er_bilinear_fwd(_p(_f32c(x)), _p(_f32c(theta)), B, F, D, bool(each), bool(plus), _p(out),
                            _stream())
    if self.op_log is not None:
      self.op_log.append(('er::bilinear_fwd_kernel', 2.0 * B * ((F - 1) * D * D + pairs * D)))
    return out

  def bilinear_bwd(self, x, theta, dout, F, D, each, plus, grads, acc=True):
    """-> dx [B, F * D]; the parameter gradients are added into (acc) or written to `grads` (a ThetaGradTable: the
    buffers in theta's order, kernel and bias per dense layer)."""
    B = x.shape[0]
    pairs = F * (F - 1) // 2
    assert dout.shape == (B, pairs if plus else pairs * D)
    dx = torch.empty_like(x)
    rows = int(self.lib.er_bilinear_grid(B, F, D, bool(each)))
    partials = torch.empty(rows * theta.numel(), dtype=torch.float32, device=x.device)
    self.ck.er_bilinear_bwd(_p(_f32c(x)), _p(_f32c(theta)), _p(_f32c(dout)), B, F, D, bool(each), bool(plus),
                            _p(dx), _p(partials), _stream())
    self.theta_grad_reduce(partials, rows, grads, 8, acc)
    if self.op_log is not None:
      self.op_log.append(('er::bilinear_bwd_kernel', 6.0 * B * ((F - 1) * D * D + pairs * D)))
    return dx

  def senet_lds_bytes(self, F, D, G, R):
    return int(self.lib.er_senet_lds_bytes(int(F), int(D), int(G), int(R)))

  def senet_epb(self, F, D, G, R, ln, bwd):
    return int(self.lib.er_senet_epb(int(F), int(D), int(G), int(R), bool(ln), bool(bwd)))

  def senet_param_count(self, F, D, G, R, ln):
    return int(self.lib.er_senet_param_count(int(F), int(D), int(G), int(R), bool(ln)))

  def senet_fwd(self, x, theta, F, D, G, R, skip, ln, want_a1=False):
    """x [B, F * D], theta: W1, b1, W2, b2 (, gamma, beta) packed -> y [B, F * D] (and a1 [B, R], the excitation's
    hidden layer after its ReLU, with want_a1)."""
    B = x.shape[0]
    assert x.shape == (B, F * D) and theta.numel() == self.senet_param_count(F, D, G, R, ln)
    y = torch.empty_like(x)
    a1 = torch.empty(B, R, dtype=torch.float32, device=x.device) if want_a1 else None
    self.ck.er_senet_fwd(_p(_f32c(x)), _p(_f32c(theta)), B, F, D, G, R, bool(skip), bool(ln), _p(y),
                         None if a1 is None else _p(a1), _stream())
    if self.op_log is not None:
      self.op_log.append(('er::senet_fwd_kernel', 2.0 * B * R * (2 * F * G + F * D)))
    return (y, a1) if want_a1 else y

  def senet_bwd(self, x, theta, dy, F, D, G, R, skip, ln, grads, acc=True):
    """-> dx [B, F * D]; the parameter gradients into `grads` as bilinear_bwd does."""
    B = x.shape[0]
    assert dy.shape == x.shape
    dx = torch.empty_like(x)
    rows = int(self.lib.er_senet_grid(B, F, D, G, R, bool(ln)))
    partials = torch.empty(rows * theta.numel(), dtype=torch.float32, device=x.device)
    self.ck.er_senet_bwd(_p(_f32c(x)), _p(_f32c(theta)), _p(_f32c(dy)), B, F, D, G, R, bool(skip), bool(ln),
                         _p(dx), _p(partials), _stream())
    self.theta_grad_reduce(partials, rows, grads, 8, acc)
    if self.op_log is not None:
      self.op_log.append(('er::senet_bwd_kernel', 6.0 * B * R * (2 * F * G + F * D)))
    return dx

  # -- K8h combining one sequence column over time (layers/keras/text_cnn.py, layers/input_layer.py)
  @staticmethod
  def _seq_view(x):
    """x [B, L_buf, D], a column of the engine's [B * L_buf, width] sequence output read in place -> its row pitch."""
    B, L, D = x.shape
    assert x.dtype == torch.float32 and x.stride(2) == 1 and x.stride(1) >= D and x.stride(0) == L * x.stride(1), \
        'a sequence column must be fp32 [B, L_buf, D] with unit column stride and every example at L_buf rows'
    return x.stride(1)

  @staticmethod
  def _i32s(values):
    return (ctypes.c_int32 * len(values))(*[int(v) for v in values])

  def text_cnn_param_count(self, D, sizes, filters):
    return int(self.lib.er_text_cnn_param_count(int(D), len(sizes), self._i32s(sizes), self._i32s(filters)))

  def text_cnn_lds_bytes(self, P, D, sizes, filters):
    return int(self.lib.er_text_cnn_lds_bytes(int(P), int(D), len(sizes), self._i32s(sizes), self._i32s(filters)))

  def text_cnn_epb(self, P, D, sizes, filters):
    """Examples per workgroup round; 0 outside the envelope (easyrec_hip.h K8h)."""
    if not 1 <= len(sizes) <= 4 or len(sizes) != len(filters):
      return 0
    return int(self.lib.er_text_cnn_epb(int(P), int(D), len(sizes), self._i32s(sizes), self._i32s(filters)))

  def text_cnn_grid(self, B, P, D, sizes, filters):
    return int(self.lib.er_text_cnn_grid(int(B), int(P), int(D), len(sizes), self._i32s(sizes), self._i32s(filters)))

  def text_cnn_fwd(self, x, theta, P, sizes, filters, relu, out=None, want_sel=False):
    """x [B, L_buf, D] (a strided column view), theta: kernel_i [k_i, D, F_i], bias_i [F_i] per filter size packed ->
    y [B, sum F_i]: the maxima over the window positions of act(conv); `out`: a [B, sum F_i] view of a wider buffer.
    want_sel: also int64 [B, sum F_i], bit p set where window position p equals the maximum."""
    B, L, D = x.shape
    ld = self._seq_view(x)
    SF = sum(int(f) for f in filters)
    assert theta.numel() == self.text_cnn_param_count(D, sizes, filters)
    y = torch.empty(B, SF, dtype=torch.float32, device=x.device) if out is None else out
    assert y.shape == (B, SF) and y.stride(1) == 1 and y.stride(0) >= SF
    sel = torch.empty(B, SF, dtype=torch.int64, device=x.device) if want_sel else None
    self.ck.er_text_cnn_fwd(_p(x), ld, L, _p(_f32c(theta)), B, int(P), D, len(sizes), self._i32s(sizes),
                            self._i32s(filters), bool(relu), _p(y), y.stride(0), _p(sel), _stream())
    if self.op_log is not None:
      self.op_log.append(('er::text_cnn_fwd_kernel', 2.0 * B * self._text_cnn_macs(P, D, sizes, filters)))
    return (y, sel) if want_sel else y

  @staticmethod
  def _text_cnn_macs(P, D, sizes, filters):
    return sum((P - k + 1) * k * D * f for k, f in zip(sizes, filters))

  def text_cnn_bwd(self, x, theta, dy, P, sizes, filters, relu, grads, acc=True, dx=None):
    """-> dx [B, L_buf, D] (`dx`: a column view of a wider buffer, whose other columns are left alone); the parameter
    gradients are added into (acc) or written to `grads` (a ThetaGradTable: kernel and bias per filter size)."""
    B, L, D = x.shape
    ld = self._seq_view(x)
    SF = sum(int(f) for f in filters)
    assert dy.shape == (B, SF) and dy.dtype == torch.float32 and dy.stride(1) == 1
    if dx is None:
      dx = torch.empty(B, L, D, dtype=torch.float32, device=x.device)
    assert dx.shape == x.shape
    lddx = self._seq_view(dx)
    rows = self.text_cnn_grid(B, P, D, sizes, filters)
    partials = torch.empty(rows * theta.numel(), dtype=torch.float32, device=x.device)
    self.ck.er_text_cnn_bwd(_p(x), ld, L, _p(_f32c(theta)), _p(dy), dy.stride(0), B, int(P), D, len(sizes),
                            self._i32s(sizes), self._i32s(filters), bool(relu), _p(dx), lddx, _p(partials), _stream())
    self.theta_grad_reduce(partials, rows, grads, 8, acc)
    if self.op_log is not None:
      self.op_log.append(('er::text_cnn_bwd_kernel', 6.0 * B * self._text_cnn_macs(P, D, sizes, filters)))
    return dx

  def seq_attn_pool_lds_bytes(self, L_buf, D, bwd):
    return int(self.lib.er_seq_attn_pool_lds_bytes(int(L_buf), int(D), bool(bwd)))

  def seq_attn_pool_epb(self, L_buf, D):
    """Examples per workgroup round; 0 outside the envelope (easyrec_hip.h K8h)."""
    return int(self.lib.er_seq_attn_pool_epb(int(L_buf), int(D)))

  def seq_attn_pool_grid(self, B, L_buf, D):
    return int(self.lib.er_seq_attn_pool_grid(int(B), int(L_buf), int(D)))

  def seq_attn_pool_fwd(self, x, seq_len, w):
    """x [B, L_buf, D] (a strided column view), seq_len int32 [B], w [D] -> the softmax-weighted sum over time [B, D]."""
    B, L, D = x.shape
    ld = self._seq_view(x)
    assert seq_len.dtype == torch.int32 and seq_len.numel() == B and seq_len.is_contiguous() and w.numel() == D
    y = torch.empty(B, D, dtype=torch.float32, device=x.device)
    self.ck.er_seq_attn_pool_fwd(_p(x), ld, _p(seq_len), _p(_f32c(w)), B, L, D, _p(y), D, _stream())
    if self.op_log is not None:
      self.op_log.append(('er::seq_attn_pool_fwd_kernel', 4.0 * B * L * D))
    return y

  def seq_attn_pool_bwd(self, x, seq_len, w, dy, grads, acc=True, dx=None):
    """-> dx [B, L_buf, D] (`dx`: a column view of a wider buffer); dw is added into (acc) or written to `grads` (a
    ThetaGradTable of w's buffer)."""
    B, L, D = x.shape
    if dx is None:
      dx = torch.empty(B, L, D, dtype=torch.float32, device=x.device)
    ld, lddx = self._seq_view(x), self._seq_view(dx)
    assert dx.shape == x.shape and dy.shape == (B, D)
    rows = self.seq_attn_pool_grid(B, L, D)
    partials = torch.empty(rows * D, dtype=torch.float32, device=x.device)
    self.ck.er_seq_attn_pool_bwd(_p(x), ld, _p(seq_len), _p(_f32c(w)), _p(_f32c(dy)), B, L, D, _p(dx), lddx, _p(partials),
                                 _stream())
    self.theta_grad_reduce(partials, rows, grads, 8, acc)
    if self.op_log is not None:
      self.op_log.append(('er::seq_attn_pool_bwd_kernel', 10.0 * B * L * D))
    return dx

  # -- K8f the head of the two-tower retrieval models (model/match_model.py)
  MATCH_MAX_D = 128

  def match_lds_bytes(self, D):
    return int(self.lib.er_match_lds_bytes(int(D)))

  def match_normalize_fwd(self, x):
    """x [R, D] -> (x * inv_norm, inv_norm [R]), inv_norm = 1 / sqrt(max(sum x^2, 1e-12)) per row."""
    R, D = x.shape
    y = torch.empty_like(x)
    inv = torch.empty(R, dtype=torch.float32, device=x.device)
    self.ck.er_match_normalize_fwd(_p(_f32c(x)), R, D, _p(y), _p(inv), _stream())
    return y, inv

  def match_normalize_bwd(self, x, inv, dy):
    R, D = x.shape
    assert dy.shape == x.shape
    dx = torch.empty_like(x)
    self.ck.er_match_normalize_bwd(_p(_f32c(x)), _p(inv), _p(_f32c(dy)), R, D, _p(dx), _stream())
    return dx

  @staticmethod
  def _match_operands(U, I, item_ids, weight):
    B, D = U.shape
    M = I.shape[0]
    assert I.shape == (M, D) and M >= B >= 1
    assert item_ids is None or (item_ids.dtype == torch.int64 and item_ids.shape == (M,) and item_ids.is_contiguous())
    assert weight is None or weight.shape == (B,)
    return B, M, D

  def match_softmax_fwd(self, U, I, inv_temperature, sim_w, sim_b, item_ids, ignore_in_batch, weight):
    """The list-wise head's forward (easyrec_hip.h K8f) -> (losses [3] = cross_entropy_loss, reg_pos_loss, sum of the
    weights; stats [4, B] = row maximum, row sum, diagonal logit, hit probability)."""
    B, M, D = self._match_operands(U, I, item_ids, weight)
    stats = torch.empty(4, B, dtype=torch.float32, device=U.device)
    partials = torch.empty(int(self.lib.er_match_grid(B)) * 3, dtype=torch.float32, device=U.device)
    losses = torch.empty(3, dtype=torch.float32, device=U.device)
    self.ck.er_match_softmax_fwd(
        _p(_f32c(U)), _p(_f32c(I)), B, M, D, float(inv_temperature), _p(sim_w), _p(sim_b), _p(item_ids),
        bool(ignore_in_batch), None if weight is None else _p(_f32c(weight)), _p(stats[0]), _p(stats[1]), _p(stats[2]),
        _p(stats[3]), _p(partials), _p(losses), _stream())
    if self.op_log is not None:
      self.op_log.append(('er::match_fwd_kernel', 2.0 * B * M * D))
    return losses, stats

  def match_softmax_bwd(self, U, I, inv_temperature, sim_w, sim_b, item_ids, ignore_in_batch, weight, stats, losses,
                        g_ce, g_reg, grads=None, acc=True):
    """-> (dU, dI); with sim_w / sim_b their gradients are added into (acc) or written to `grads` (a ThetaGradTable of
    the two one-float buffers)."""
    B, M, D = self._match_operands(U, I, item_ids, weight)
    dU, dI = torch.empty_like(U), torch.empty_like(I)
    rows = int(self.lib.er_match_grid(B))
    partials = torch.empty(rows * 2, dtype=torch.float32, device=U.device)
    self.ck.er_match_softmax_bwd(
        _p(_f32c(U)), _p(_f32c(I)), B, M, D, float(inv_temperature), _p(sim_w), _p(sim_b), _p(item_ids),
        bool(ignore_in_batch), None if weight is None else _p(_f32c(weight)), _p(stats[0]), _p(stats[1]), _p(stats[3]),
        _p(losses), _p(_f32c(g_ce)), _p(_f32c(g_reg)), _p(dU), _p(dI), _p(partials), _stream())
    if grads is not None:
      self.theta_grad_reduce(partials, rows, grads, 1, acc)
    if self.op_log is not None:
      self.op_log.append(('er::match_bwd_kernel', 8.0 * B * M * D))
    return dU, dI

  def match_rank_counts(self, U, I, inv_temperature, sim_w, sim_b, item_ids, ignore_in_batch):
    """-> (c_in [B], c_neg [B]) int32: how many in-batch columns / extra negatives rank above each row's positive."""
    B, M, D = self._match_operands(U, I, item_ids, None)
    c_in = torch.empty(B, dtype=torch.int32, device=U.device)
    c_neg = torch.empty(B, dtype=torch.int32, device=U.device)
    self.ck.er_match_rank_counts(
        _p(_f32c(U)), _p(_f32c(I)), B, M, D, float(inv_temperature), _p(sim_w), _p(sim_b), _p(item_ids),
        bool(ignore_in_batch), _p(c_in), _p(c_neg), _stream())
    return c_in, c_neg

  # -- K1b negative_sampler_in_memory (input/neg_sampler.py)
  NEG_SAMPLE_MAX_COLS = 32

  def neg_sample_lds_bytes(self, B):
    return int(self.lib.er_neg_sample_lds_bytes(int(B)))

  def neg_sample(self, table_ids, batch_ids, N, step, step_offset, seed, columns, sel):
    """The draw of easyrec_hip.h K1b at step *step + step_offset.  columns: [(table column [n], the batch's column [B],
    its extended buffer [B + N])], int64 or fp32; sel: int32 [N]."""
    n, B = table_ids.numel(), batch_ids.numel()
    assert table_ids.dtype == torch.int64 and batch_ids.dtype == torch.int64 and step.dtype == torch.int64
    assert table_ids.is_contiguous() and batch_ids.is_contiguous()
    assert sel.dtype == torch.int32 and sel.numel() == N and sel.is_contiguous()
    nc = len(columns)
    tabs, bats, outs, sizes = [], [], [], []
    for tab, bat, out in columns:
      assert tab.dtype == bat.dtype == out.dtype and tab.dtype in (torch.int64, torch.float32), tab.dtype
      assert tab.numel() == n and bat.numel() == B and out.numel() == B + N
      assert tab.is_contiguous() and bat.is_contiguous() and out.is_contiguous()
      tabs.append(tab.data_ptr())
      bats.append(bat.data_ptr())
      outs.append(out.data_ptr())
      sizes.append(tab.element_size())
    ptrs = ctypes.c_void_p * max(nc, 1)
    self.ck.er_neg_sample(
        _p(table_ids), n, _p(batch_ids), B, int(N), _p(step), int(step_offset), int(seed) & 0xFFFFFFFFFFFFFFFF, ptrs(*tabs),
        ptrs(*bats), ptrs(*outs), (ctypes.c_int32 * max(nc, 1))(*sizes), nc, _p(sel), _stream())

  # -- K1c negative_sampler: the weighted draw with replacement (input/neg_sampler.py)
  def neg_sample_weighted_lds_bytes(self, B):
    return int(self.lib.er_neg_sample_weighted_lds_bytes(int(B)))

  def neg_sample_weighted(self, alias_tab, table_ids, batch_ids, N, step, step_offset, seed, columns, sel):
    """The draw of easyrec_hip.h K1c at step *step + step_offset.  alias_tab: int64 [n] holding the uint64 records
    (neg_sampler.alias_table); the other arguments as neg_sample."""
    n, B = table_ids.numel(), batch_ids.numel()
    assert alias_tab.dtype == torch.int64 and alias_tab.numel() == n and alias_tab.is_contiguous()
    assert table_ids.dtype == torch.int64 and batch_ids.dtype == torch.int64 and step.dtype == torch.int64
    assert table_ids.is_contiguous() and batch_ids.is_contiguous()
    assert sel.dtype == torch.int32 and sel.numel() == N and sel.is_contiguous()
    nc = len(columns)
    tabs, bats, outs, sizes = [], [], [], []
    for tab, bat, out in columns:
      assert tab.dtype == bat.dtype == out.dtype and tab.dtype in (torch.int64, torch.float32), tab.dtype
      assert tab.numel() == n and bat.numel() == B and out.numel() == B + N
      assert tab.is_contiguous() and bat.is_contiguous() and out.is_contiguous()
      tabs.append(tab.data_ptr())
      bats.append(bat.data_ptr())
      outs.append(out.data_ptr())
      sizes.append(tab.element_size())
    ptrs = ctypes.c_void_p * max(nc, 1)
    self.ck.er_neg_sample_weighted(
        _p(alias_tab), _p(table_ids), n, _p(batch_ids), B, int(N), _p(step), int(step_offset),
        int(seed) & 0xFFFFFFFFFFFFFFFF, ptrs(*tabs), ptrs(*bats), ptrs(*outs), (ctypes.c_int32 * max(nc, 1))(*sizes), nc,
        _p(sel), _stream())

  # -- K9k full-corpus top-K search and hit count (core/knn.py, core/hit_rate.py)
  def knn_lds_bytes(self, D, K):
    return int(self.lib.er_knn_lds_bytes(int(D), int(K)))

  def knn_workspace_bytes(self, nq, K, slices=0):
    return int(self.lib.er_knn_workspace_bytes(int(nq), int(K), int(slices)))

  def knn_norms(self, items):
    """items [n, D] -> xx [n]: the fmaf chain over x_d^2 of every row."""
    n, D = items.shape
    xx = torch.empty(n, dtype=torch.float32, device=items.device)
    self.ck.er_knn_norms(_p(_f32c(items)), n, D, _p(xx), _stream())
    return xx

  def knn_search(self, queries, items, xx, table_ids, K, metric, slices=0):
    """The search of easyrec_hip.h K9k -> (ids int64 [nq, K], rows int32 [nq, K], dist fp32 [nq, K])."""
    nq, D = queries.shape
    n = items.shape[0]
    assert items.shape == (n, D) and items.dtype == torch.float32 and items.is_contiguous()
    assert table_ids.dtype == torch.int64 and table_ids.shape == (n,) and table_ids.is_contiguous()
    assert metric == 1 or (xx is not None and xx.shape == (n,) and xx.dtype == torch.float32 and xx.is_contiguous())
    nbytes = self.knn_workspace_bytes(nq, K, slices)
    if nbytes <= 0:
      raise RuntimeError('er_knn_search: nq %d, K %d, slices %d outside the envelope' % (nq, K, slices))
    dev = queries.device
    work = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    ids = torch.empty(nq, K, dtype=torch.int64, device=dev)
    rows = torch.empty(nq, K, dtype=torch.int32, device=dev)
    dist = torch.empty(nq, K, dtype=torch.float32, device=dev)
    self.ck.er_knn_search(
        _p(_f32c(queries)), _p(items), None if xx is None else _p(xx), _p(table_ids), nq, n, D, int(K), int(metric),
        int(slices), _p(work), _p(ids), _p(rows), _p(dist), _stream())
    if self.op_log is not None:
      self.op_log.append(('er::knn_scan_kernel', 2.0 * nq * n * D))
    return ids, rows, dist

  def knn_hits(self, ids, user_emb_num, gt_offsets, gt_ids):
    """ids int64 [U, I, K], user_emb_num int32 [U], gt_offsets int64 [U + 1], gt_ids int64 -> (hits, gt_count) int32 [U]"""
    U, I, K = ids.shape
    assert ids.dtype == torch.int64 and ids.is_contiguous()
    assert user_emb_num.dtype == torch.int32 and user_emb_num.shape == (U,) and user_emb_num.is_contiguous()
    assert gt_offsets.dtype == torch.int64 and gt_offsets.shape == (U + 1,) and gt_offsets.is_contiguous()
    assert gt_ids.dtype == torch.int64 and gt_ids.is_contiguous()
    hits = torch.empty(U, dtype=torch.int32, device=ids.device)
    gt_count = torch.empty(U, dtype=torch.int32, device=ids.device)
    self.ck.er_knn_hits(_p(ids), _p(user_emb_num), _p(gt_offsets), _p(gt_ids), U, I, K, _p(hits),
                        _p(gt_count), _stream())
    return hits, gt_count

  # -- K8g MIND's capsule layer and label-aware attention (layers/capsule_layer.py, model/mind.py)
  CAPSULE_MAX_K = 8
  MIND_ATT_MAX_E = 128

  def capsule_lds_bytes(self, S, D, E, K):
    return int(self.lib.er_capsule_lds_bytes(int(S), int(D), int(E), int(K)))

  def capsule_grid(self, B):
    return int(self.lib.er_capsule_grid(int(B)))

  def capsule_fwd(self, hist, seq_len, Smat, logits0, S, K, num_iters, scale, squash_pow, scale_ratio, const_caps):
    """hist [B, L, D], seq_len [B] int32, Smat [D, E], logits0 [B, S, K] (per example) or [S, K] (shared) ->
    (high_capsules [B, K, E], num_caps [B] int32, W [B, S, K]: the last iteration's routing weights)."""
    B, L, D = hist.shape
    E = Smat.shape[1]
    assert Smat.shape == (D, E) and seq_len.dtype == torch.int32 and seq_len.shape == (B,)
    assert logits0.shape in ((B, S, K), (S, K)) and logits0.is_contiguous() and logits0.dtype == torch.float32
    stride = S * K if logits0.dim() == 3 else 0
    high = torch.empty(B, K, E, dtype=torch.float32, device=hist.device)
    ncaps = torch.empty(B, dtype=torch.int32, device=hist.device)
    W = torch.empty(B, S, K, dtype=torch.float32, device=hist.device)
    self.ck.er_capsule_fwd(_p(_f32c(hist)), _p(seq_len), _p(_f32c(Smat)), _p(logits0), stride, B, L, S, D, E, K,
                           int(num_iters), float(scale), float(squash_pow), float(scale_ratio), bool(const_caps),
                           _p(high), _p(ncaps), _p(W), _stream())
    if self.op_log is not None:
      self.op_log.append(('er::capsule_fwd_kernel', 2.0 * B * S * E * (D + K * (2 * num_iters - 1))))
    return high, ncaps, W

  def capsule_bwd(self, hist, seq_len, Smat, W, d_high, squash_pow, scale_ratio, const_caps, grads, dhist=None,
                  acc_h=False, acc=True):
    """-> dhist [B, L, D] (written, or added into with acc_h); capsule/S's gradient is added into (acc) or written to
    `grads` (a ThetaGradTable of the one [D, E] buffer)."""
    B, L, D = hist.shape
    _, S, K = W.shape
    E = Smat.shape[1]
    assert d_high.shape == (B, K, E)
    if dhist is None:
      assert not acc_h
      dhist = torch.empty_like(hist)
    assert dhist.shape == hist.shape and dhist.is_contiguous()
    rows = self.capsule_grid(B)
    partials = torch.empty(rows * D * E, dtype=torch.float32, device=hist.device)
    self.ck.er_capsule_bwd(_p(_f32c(hist)), _p(seq_len), _p(_f32c(Smat)), _p(_f32c(W)), _p(_f32c(d_high)), B, L,
                           S, D, E, K, float(squash_pow), float(scale_ratio), bool(const_caps), _p(dhist),
                           bool(acc_h), _p(partials), _stream())
    self.theta_grad_reduce(partials, rows, grads, 1, acc)
    if self.op_log is not None:
      self.op_log.append(('er::capsule_bwd_kernel', 2.0 * B * S * E * (3 * D + 2 * K)))
    return dhist

  def mind_attention_fwd(self, interests, pos_item, num_caps, simi_pow):
    """interests [B, K, E], pos_item [B, E], num_caps [B] int32 -> (user_emb [B, E], user_interests [B, K, E], weights
    [B, K])."""
    B, K, E = interests.shape
    assert pos_item.shape == (B, E) and num_caps.dtype == torch.int32 and num_caps.shape == (B,)
    emb = torch.empty(B, E, dtype=torch.float32, device=interests.device)
    ui = torch.empty_like(interests)
    w = torch.empty(B, K, dtype=torch.float32, device=interests.device)
    self.ck.er_mind_attention_fwd(_p(_f32c(interests)), _p(_f32c(pos_item)), _p(num_caps), B, K, E,
                                  float(simi_pow), _p(emb), _p(ui), _p(w), _stream())
    return emb, ui, w

  def mind_attention_bwd(self, interests, pos_item, num_caps, weights, d_emb, d_ui, simi_pow):
    """-> (d_interests [B, K, E], d_pos_item [B, E]); d_ui: the gradient of user_interests, or None."""
    B, K, E = interests.shape
    assert d_emb.shape == (B, E) and (d_ui is None or d_ui.shape == (B, K, E))
    di = torch.empty_like(interests)
    dp = torch.empty_like(pos_item)
    self.ck.er_mind_attention_bwd(_p(_f32c(interests)), _p(_f32c(pos_item)), _p(num_caps), _p(weights),
                                  _p(_f32c(d_emb)), None if d_ui is None else _p(_f32c(d_ui)), B, K, E,
                                  float(simi_pow), _p(di), _p(dp), _stream())
    return di, dp

  # -- K1b hash-table (KV) embedding tables
  def kv_create(self, var_rows, capacity, seed, init_mean, init_stddev, filter_freq=0, steps_to_live=0, step=None):
    """The map of one KV table whose arena is `var_rows` ([capacity, dim] view of the table group's storage).
    filter_freq > 1: keys get their row once seen that often (the map then tracks every id SEEN: 4x the slots);
    steps_to_live > 0: every training lookup stamps the key with `step` (int64 device counter) for evict at save time."""
    dev = var_rows.device
    filter_freq, steps_to_live = int(filter_freq), int(steps_to_live)
    slots = 1
    while slots < (8 if filter_freq > 1 else 2) * int(capacity):
      slots *= 2
    assert slots <= (1 << 31), 'hash-table embedding: %d map slots (the kernels count slots and rows in 32 bits)' % slots
    kv = {'keys': torch.full((slots,), -1, dtype=torch.int64, device=dev),
          'rows': torch.full((slots,), -1, dtype=torch.int32, device=dev),
          'next_row': torch.zeros(1, dtype=torch.int32, device=dev),
          'overflow': torch.zeros(1, dtype=torch.int32, device=dev),
          'capacity': int(capacity), 'var': var_rows, 'dim': int(var_rows.shape[1]), 'seed': int(seed) & ((1 << 63) - 1),
          'mean': float(init_mean), 'stddev': float(init_stddev), 'filter_freq': filter_freq,
          'steps_to_live': steps_to_live, 'freq': None, 'version': None, 'n_keys': None, 'step': None}
    if filter_freq > 1:
      kv['freq'] = torch.zeros(slots, dtype=torch.int32, device=dev)
      kv['n_keys'] = torch.zeros(1, dtype=torch.int32, device=dev)
    if steps_to_live > 0:
      assert step is not None and step.dtype == torch.int64, 'steps_to_live needs the device step counter'
      kv['version'] = torch.zeros(slots, dtype=torch.int32, device=dev)
      kv['step'] = step
    return kv

  @staticmethod
  def _kv_job(kv, ids, rows_out, limit=None):
    return KvJob(ids.data_ptr(), ids.numel(), kv['keys'].data_ptr(), kv['rows'].data_ptr(), kv['keys'].numel(),
                 kv['next_row'].data_ptr(), kv['var'].data_ptr(), kv['seed'], rows_out.data_ptr(),
                 kv['overflow'].data_ptr(), kv['capacity'], kv['dim'], kv['mean'], kv['stddev'], _p(limit),
                 _p(kv['freq']), _p(kv['version']), _p(kv['n_keys']), _p(kv['step']), kv['filter_freq'],
                 kv['var'].stride(0) if kv['var'].stride(0) != kv['dim'] else 0)

  def kv_translate(self, kv, ids, rows_out, insert):
    """rows_out[i] = arena row of ids[i] (-1: no row); insert: a training lookup (unseen ids get a row, or - filtered
    tables - a count)."""
    assert ids.dtype == torch.int64 and rows_out.dtype == torch.int64 and ids.is_contiguous() and rows_out.is_contiguous()
    assert ids.numel() == rows_out.numel()
    job = self._kv_job(kv, ids, rows_out)
    self.ck.er_kv_translate_job(ctypes.byref(job), insert, _stream())

  def kv_jobs_create(self, jobs):
    """jobs: [(kv, ids, rows_out[, n_limit])] -> the device-resident descriptor table of er_kv_translate_multi (built
    once).  n_limit: int32 device scalar = the number of valid ids of the step (ragged lists in fixed buffers)."""
    n = len(jobs)
    arr = (KvJob * n)()
    starts = [0]
    for i, job in enumerate(jobs):
      kv, ids, rows_out = job[:3]
      limit = job[3] if len(job) > 3 else None
      assert limit is None or (limit.dtype == torch.int32 and limit.numel() == 1)
      assert ids.dtype == torch.int64 and rows_out.dtype == torch.int64 and ids.is_contiguous() and rows_out.is_contiguous()
      arr[i] = self._kv_job(kv, ids, rows_out, limit)
      starts.append(starts[-1] + (ids.numel() + 255) // 256)
    dev = jobs[0][1].device
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    blk = torch.tensor(starts, dtype=torch.int32, device=dev)
    return {'table': table, 'blk_start': blk, 'n': n, 'blocks': starts[-1], 'jobs': jobs}

  def kv_translate_multi(self, handle, insert):
    if handle['blocks'] == 0:
      return
    self.ck.er_kv_translate_multi(_p(handle['table']), _p(handle['blk_start']), handle['n'], handle['blocks'],
                                  insert, _stream())

  def kv_route_create(self, jobs, world):
    """Embedding-parallel hash tables: jobs [(ids, rows_out[, n_limit])] -> the buffers and descriptor table of
    er_kv_bucket / er_kv_unbucket.  send / recv / owner_rows / back: int64 [world, C] with C = the jobs' id counts
    summed (job j's region of every owner's block is [off_j, off_j + n_j): a job fits even if all its ids have one owner)."""
    n = len(jobs)
    dev = jobs[0][0].device
    arr = (KvRouteJob * n)()
    starts, offs, slots = [0], [0], []
    for i, job in enumerate(jobs):
      ids, rows_out = job[:2]
      limit = job[2] if len(job) > 2 else None
      assert ids.dtype == torch.int64 and rows_out.dtype == torch.int64 and ids.is_contiguous() and rows_out.is_contiguous()
      assert ids.numel() == rows_out.numel() and (limit is None or (limit.dtype == torch.int32 and limit.numel() == 1))
      slot = torch.full((ids.numel(),), -1, dtype=torch.int32, device=dev)
      slots.append(slot)
      arr[i] = KvRouteJob(ids.data_ptr(), ids.numel(), 0 if limit is None else limit.data_ptr(), rows_out.data_ptr(),
                          slot.data_ptr(), offs[-1])
      starts.append(starts[-1] + (ids.numel() + 255) // 256)
      offs.append(offs[-1] + ids.numel())
    C = max(offs[-1], 1)
    buf = lambda: torch.full((world, C), -1, dtype=torch.int64, device=dev)
    return {'table': torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev),
            'blk_start': torch.tensor(starts, dtype=torch.int32, device=dev), 'n': n, 'blocks': starts[-1], 'world': int(world),
            'C': C, 'offs': offs, 'slots': slots, 'jobs': jobs, 'send': buf(), 'recv': buf(), 'owner_rows': buf(), 'back': buf(),
            'counts': torch.zeros(n * world, dtype=torch.int32, device=dev)}

  def kv_bucket(self, h):
    if h['blocks']:
      self.ck.er_kv_bucket(_p(h['table']), _p(h['blk_start']), h['n'], h['blocks'], h['world'], h['C'],
                           _p(h['send']), _p(h['counts']), _stream())

  def kv_unbucket(self, h):
    if h['blocks']:
      self.ck.er_kv_unbucket(_p(h['table']), _p(h['blk_start']), h['n'], h['blocks'], h['world'],
                             h['C'], _p(h['back']), _stream())

  def kv_export(self, kv):
    """(keys ascending, arena rows) of the table's materialised ids (host sync)."""
    n_max = kv['capacity']
    keys = torch.empty(n_max, dtype=torch.int64, device=kv['keys'].device)
    rows = torch.empty(n_max, dtype=torch.int32, device=kv['keys'].device)
    count = torch.zeros(1, dtype=torch.int32, device=kv['keys'].device)
    self.ck.er_kv_export(_p(kv['keys']), _p(kv['rows']), kv['keys'].numel(), _p(keys), _p(rows),
                         _p(count), _stream())
    n = int(count.item())
    keys, rows = keys[:n], rows[:n]
    order = torch.argsort(keys)
    return keys[order], rows[order].to(torch.int64)

  def kv_export_all(self, kv):
    """Every key the map holds, ascending: (keys, arena rows (-1: no row yet), freq, version) (host sync)."""
    slots, dev = kv['keys'].numel(), kv['keys'].device
    # (one record per map slot: a launch that crosses the load-factor threshold may claim more than slots / 2 of them while
    # raising only the sticky overflow flag - the export must stay in bounds whatever the map holds)
    n_max = slots
    keys = torch.empty(n_max, dtype=torch.int64, device=dev)
    rows, freq, version = (torch.empty(n_max, dtype=torch.int32, device=dev) for _ in range(3))
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    self.ck.er_kv_export_all(_p(kv['keys']), _p(kv['rows']), _p(kv['freq']), _p(kv['version']),
                             slots, _p(keys), _p(rows), _p(freq), _p(version), _p(count), _stream())
    n = int(count.item())
    order = torch.argsort(keys[:n])
    return keys[:n][order], rows[:n][order].to(torch.int64), freq[:n][order], version[:n][order]

  def kv_rebuild(self, kv, keys, rows, freq=None, version=None):
    """Replace the map's content: distinct `keys` with their arena `rows` (-1: tracked, no row yet), counts and stamps.
    The rows in use become 0 .. (number of rows >= 0) - 1: the caller has laid the arena out that way."""
    dev = kv['keys'].device
    keys = keys.to(dev, torch.int64).contiguous()
    rows32 = rows.to(dev, torch.int32).contiguous()
    kv['keys'].fill_(-1)
    kv['rows'].fill_(-1)
    if kv['freq'] is not None:
      kv['freq'].zero_()
      freq = None if freq is None else freq.to(dev, torch.int32).contiguous()
    if kv['version'] is not None:
      kv['version'].zero_()
      version = None if version is None else version.to(dev, torch.int32).contiguous()
    self.ck.er_kv_rebuild(_p(keys), _p(rows32), _p(freq) if kv['freq'] is not None else None,
                          _p(version) if kv['version'] is not None else None, keys.numel(),
                          _p(kv['keys']), _p(kv['rows']), _p(kv['freq']), _p(kv['version']),
                          kv['keys'].numel(), _p(kv['overflow']), _stream())
    kv['next_row'].fill_(int((rows32 >= 0).sum().item()))
    if kv['n_keys'] is not None:
      kv['n_keys'].fill_(keys.numel())

  # -- K9b CIN (xDeepFM)
  def cin_outer_fwd(self, xi, strides, H, x0, z):
    """z[(b, d), h * H0 + m] = xi[b, h, d] * x0[b, m, d]; xi addressed by strides = (stride_b, stride_h, stride_d)."""
    B, H0, D = x0.shape
    assert z.shape == (B * D, H * H0) and z.is_contiguous() and x0.is_contiguous()
    self.ck.er_cin_outer_fwd(_p(xi), strides[0], strides[1], strides[2], H, _p(x0), H0, D, B, _p(z),
                             _stream())

  def cin_act_pool_fwd(self, c, bias, B, D, pooled, col0):
    """c [B * D, N] <- relu(c + bias) in place; pooled[:, col0 : col0 + N] = its sum over d."""
    N = c.shape[1]
    assert c.is_contiguous() and pooled.stride(1) == 1
    self.ck.er_cin_act_pool_fwd(_p(c), _p(bias), B, D, N, _p(pooled), pooled.stride(0), col0, _stream())

  def cin_act_pool_bwd(self, fm, dpooled, col0, dnext, B, D, dc):
    N = fm.shape[1]
    assert fm.is_contiguous() and dc.is_contiguous() and dpooled.stride(1) == 1 and (dnext is None or dnext.is_contiguous())
    self.ck.er_cin_act_pool_bwd(_p(fm), _p(dpooled), dpooled.stride(0), col0, _p(dnext), B, D, N, _p(dc),
                                _stream())

  def cin_outer_bwd(self, dz, xi, strides, H, x0, dxi, add_xi, dx0):
    B, H0, D = x0.shape
    assert dz.shape == (B * D, H * H0) and dz.is_contiguous() and dx0.is_contiguous()
    self.ck.er_cin_outer_bwd(_p(dz), _p(xi), strides[0], strides[1], strides[2], H, _p(x0), H0, D, B, _p(dxi),
                             add_xi, _p(dx0), _stream())

  # -- K9 MLP pieces
  def bn_act_fwd(self, x, bias, gamma, beta, use_bn, eps, momentum, moving_mean, moving_var, act):
    B, N = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(N, dtype=torch.float32, device=x.device) if use_bn else None
    invstd = torch.empty(N, dtype=torch.float32, device=x.device) if use_bn else None
    self.ck.er_bn_act_fwd(_p(_f32c(x)), _p(bias), _p(gamma), _p(beta), B, N, int(use_bn),
                          eps, momentum, _p(moving_mean), _p(moving_var),
                          int(act), _p(y), _p(mean), _p(invstd), _stream())
    return y, mean, invstd

  def copy_multi(self, pairs):
    """[(dst, src)] device tensors (same byte size, contiguous) -> all copies in one launch (er_copy_multi)."""
    n = len(pairs)
    if n == 0:
      return
    srcs = (ctypes.c_void_p * n)(*[s_.data_ptr() for _, s_ in pairs])
    dsts = (ctypes.c_void_p * n)(*[d.data_ptr() for d, _ in pairs])
    nb = (ctypes.c_int64 * n)(*[s_.numel() * s_.element_size() for _, s_ in pairs])
    self.ck.er_copy_multi(srcs, dsts, nb, n, _stream())

  concat_pitch = os.environ.get('EASYREC_AMD_CONCAT_PITCH', '1') != '0'  # A/B switch

  def concat_cols(self, parts, bf16_state=None):
    """torch.cat(parts, dim=1) of 2-D fp32 blocks (unit inner stride) as one library launch.  bf16_state (a Bf16Shadows):
    the launch also writes the bf16 copy the next contraction reads, registered there."""
    n = len(parts)
    B = parts[0].shape[0]
    for t in parts:
      assert t.dim() == 2 and t.shape[0] == B and t.stride(1) == 1 and t.dtype == torch.float32
    # rows at a pitch that is a multiple of four floats (DeepFM's [wide | fm | deep] is 81 wide): the consumers' GEMMs
    # then see a 16-byte aligned operand and take their branch-free 16-byte loads instead of the masked scalar path
    width = sum(t.shape[1] for t in parts)
    pitch = (width + 3) // 4 * 4 if self.concat_pitch else width
    out = torch.empty(B, pitch, dtype=torch.float32, device=parts[0].device)[:, :width]
    outb = None
    if bf16_state is not None and n <= 8:
      outb = torch.empty(B, bf16_state.pad8(width), dtype=torch.bfloat16, device=out.device)  # (k-tail zeroed by the kernel)
      bf16_state.register(out, outb)
    for i in range(0, n, 8):  # (more than 8 parts: several launches into column blocks of `out`)
      chunk = parts[i:i + 8]
      col0 = sum(t.shape[1] for t in parts[:i])
      dst = out[:, col0:]
      pp = (ctypes.c_void_p * len(chunk))(*[t.data_ptr() for t in chunk])
      ww = (ctypes.c_int32 * len(chunk))(*[t.shape[1] for t in chunk])
      ll = (ctypes.c_int32 * len(chunk))(*[t.stride(0) for t in chunk])
      self.ck.er_concat_cols_b16(pp, ww, ll, len(chunk), B, _p(dst), out.stride(0), _p(outb),
                                 0 if outb is None else outb.stride(0), _stream())
    return out

  def bn_act_bwd(self, x, bias, gamma, y, mean, invstd, dy, use_bn, act, need_bias, need_affine, into=None,
                 partial=None, beta=None, bf16_state=None):
    """into = (dbias_buf, dgamma_buf, dbeta_buf) (each may be None): accumulate the parameter gradients
    into those buffers (slices of the flat gradient buffer) instead of returning new tensors.
    partial: column sums [gemm_row_tiles(B)][N][2] already produced by gemm_bn_bwd (skips that pass).
    bf16_state (a Bf16Shadows): the launch also writes dx's bf16 copy, registered there for the input-gradient contraction."""
    B, N = x.shape
    dx = torch.empty_like(x)
    dev = x.device
    dxb = bf16_state.new_copy(dx) if bf16_state is not None else None
    ldb = 0 if dxb is None else dxb.stride(0)
    acc = into is not None
    if acc:
      dbias, dgamma, dbeta = into
    else:
      dbias = torch.empty(N, dtype=torch.float32, device=dev) if need_bias else None
      dgamma = torch.empty(N, dtype=torch.float32, device=dev) if need_affine else None
      dbeta = torch.empty(N, dtype=torch.float32, device=dev) if need_affine else None
    assert dy.dim() == 2 and dy.stride(1) == 1 and dy.dtype == torch.float32
    if partial is not None:
      self.ck.er_bn_act_bwd_from_partials_ld_b16(_p(x), _p(bias), _p(gamma), _p(y), _p(mean), _p(invstd), _p(dy),
                                                 dy.stride(0), B, N, int(use_bn), int(act), _p(partial),
                                                 self.gemm_row_tiles(B), _p(dx), _p(dbias), _p(dgamma),
                                                 _p(dbeta), int(acc), _p(dxb), ldb, _stream())
    else:  # (dy may be a column block of a wider gradient - ConcatFn's backward -: read in place)
      self.ck.er_bn_act_bwd_ld_b16(_p(x), _p(bias), _p(gamma), _p(y), _p(mean), _p(invstd), _p(dy),
                                   dy.stride(0), B, N, int(use_bn), int(act), _p(dx), _p(dbias),
                                   _p(dgamma), _p(dbeta), int(acc), _p(dxb), ldb, _stream())
    if acc:
      return dx, None, None, None
    return dx, dbias, dgamma, dbeta

  def colsum(self, x, out=None, accumulate=False):
    """out[j] (+)= sum_i x[i, j]; out: e.g. a bias' slice of the flat gradient buffer."""
    rows, cols = x.shape
    if out is None:
      assert not accumulate
      out = torch.empty(cols, dtype=torch.float32, device=x.device)
    self.ck.er_colsum_acc(_p(x), rows, cols, x.stride(0), _p(out), accumulate, _stream())
    return out

  def dice_fwd(self, x, alpha, eps, momentum, moving_mean, moving_var):
    B, N = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(N, dtype=torch.float32, device=x.device)
    invstd = torch.empty(N, dtype=torch.float32, device=x.device)
    self.ck.er_dice_fwd(_p(_f32c(x)), _p(alpha), B, N, eps, momentum,
                        _p(moving_mean), _p(moving_var), _p(y), _p(mean), _p(invstd), _stream())
    return y, mean, invstd

  def dice_bwd(self, x, alpha, mean, invstd, dy):
    B, N = x.shape
    dx = torch.empty_like(x)
    dalpha = torch.empty(N, dtype=torch.float32, device=x.device)
    self.ck.er_dice_bwd(_p(x), _p(alpha), _p(mean), _p(invstd), _p(_f32c(dy)), B, N, _p(dx), _p(dalpha),
                        _stream())
    return dx, dalpha

  # -- K10 loss / scalars
  def sigmoid_ce(self, logits, labels, weights, loss_scale=1.0):
    """Returns (loss [1], dlogits [B], probs [B])."""
    B = logits.numel()
    dev = logits.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    dlogits = torch.empty(B, dtype=torch.float32, device=dev)
    probs = torch.empty(B, dtype=torch.float32, device=dev)
    self.ck.er_sigmoid_ce_fwd_bwd(_p(_f32c(logits)), _p(_f32c(labels)), _p(weights), B,
                                  loss_scale, _p(loss), _p(dlogits), _p(probs), _stream())
    return loss, dlogits, probs

  def sigmoid_ce_multi(self, heads):
    """heads: [(logits, labels, weights or None, loss_scale)] -> [(loss [1], dlogits [B])] in one launch."""
    arr = (CeHead * len(heads))()
    outs, keep = [], []
    for q, (logits, labels, weights, scale) in zip(arr, heads):
      z, y = _f32c(logits), _f32c(labels)
      B = z.numel()
      loss = torch.empty(1, dtype=torch.float32, device=z.device)
      dz = torch.empty(B, dtype=torch.float32, device=z.device)
      q.logits, q.labels, q.weights = z.data_ptr(), y.data_ptr(), _p(weights)
      q.B, q.loss_scale = B, float(scale)
      q.loss_out, q.dlogits, q.probs_out = loss.data_ptr(), dz.data_ptr(), None
      outs.append((loss, dz))
      keep.append((z, y))
    self.ck.er_sigmoid_ce_multi(arr, len(heads), _stream())
    return outs

  def total_loss(self, reg_emb, reg_dense, losses, reports, reg_out, total_out):
    n = len(losses)
    src = (ctypes.c_void_p * max(n, 1))(*[t.data_ptr() for t in losses])
    dst = (ctypes.c_void_p * max(n, 1))(*[t.data_ptr() for t in reports])
    self.ck.er_total_loss(_p(reg_emb), _p(reg_dense), src, dst, n, _p(reg_out), _p(total_out), _stream())

  def reg_total_loss(self, emb_partials, emb_scale, dense_partials, losses, reports, reg_out, total_out):
    """reg_out = emb_scale * sum(emb_partials) + sum(dense_partials); total_out = reg_out + sum(losses); reports[i] =
    losses[i].  Either partial array may be None.  One launch (er_reg_total_loss)."""
    n = len(losses)
    assert n <= 8
    src = (ctypes.c_void_p * max(n, 1))(*[t.data_ptr() for t in losses])
    dst = (ctypes.c_void_p * max(n, 1))(*[t.data_ptr() for t in reports])
    n_part = 0 if emb_partials is None else emb_partials.numel()
    n_dense = 0 if dense_partials is None else dense_partials.numel()
    self.ck.er_reg_total_loss(_p(emb_partials), n_part, emb_scale, _p(dense_partials), n_dense, src, dst, n,
                              _p(reg_out), _p(total_out), _stream())

  # the binary head of a rank model (dense(K -> 1) + sigmoid cross entropy + their gradients) as ONE launch, its dW / db
  # partial sums folded into the loss tail's launch: layers/dnn.py dense(head=True), builders/loss_builder.py
  fused_head = os.environ.get('EASYREC_AMD_FUSED_HEAD', '1') != '0'  # A/B switch

  def head_sigmoid_ce(self, x, w, b, labels, loss_scale, src=None, logits=None):
    """er_head_sigmoid_ce: x [B, K] (row stride >= K), w [K, 1], b [1] or None, labels [B] -> dict(logits [B, 1], probs [B],
    dlogits [B], dx [B, K], loss_partials [T], wb_partials [T, K + 1], bn_partials [T, K, 2] or None); the loss is
    loss_scale * sum(loss_partials) / B (loss_tail).  src: the BnSource of x (x is its activation output)."""
    B, K = x.shape
    dev = x.device
    T = (B + 63) // 64
    f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
    out = {'logits': logits if logits is not None else f(B, 1), 'probs': f(B), 'dlogits': f(B), 'dx': f(B, K), 'loss_partials': f(T), 'wb_partials': f(T, K + 1),
           'bn_partials': None}
    sz = smean = sinv = None
    sld, sact = 0, ACT_NONE
    if src is not None:
      assert src.y is not None and src.y.data_ptr() == x.data_ptr() and src.zbias is None
      out['bn_partials'] = f(T, K, 2)
      sz, smean, sinv, sld, sact = src.z, src.mean, src.invstd, src.z.stride(0), src.act
    self.ck.er_head_sigmoid_ce(_p(x), x.stride(0), _p(w), _p(b), _p(_f32c(labels)), B, K, loss_scale,
                               _p(out['logits']), _p(out['probs']), _p(out['dlogits']), _p(out['dx']),
                               _p(out['loss_partials']), _p(out['wb_partials']), _p(sz), sld, _p(smean),
                               _p(sinv), int(sact), _p(out['bn_partials']), _stream())
    return out

  def loss_tail(self, emb_partials, emb_scale, dense_partials, losses, reports, reg_out, total_out, jobs=(), defer=False):
    """reg_total_loss whose task losses may be PartialLoss records (per-workgroup partial sums left by head_sigmoid_ce)
    and which also runs small column-sum jobs [(partial [P, ld], dst [n_cols], n_cols)]: dst[j] += sum_p partial[p, j].
    defer: not launched now - the step's fused tail runs it as one workgroup of its first launch (emb_bwd_fused(tail=...));
    whoever does not get that far calls flush_loss_tail() before anything reads the losses or the gradient buffer."""
    n = len(losses)
    assert n <= 8 and len(jobs) <= 4
    src = (ctypes.c_void_p * max(n, 1))()
    dst = (ctypes.c_void_p * max(n, 1))(*[t.data_ptr() for t in reports])
    parts = (ctypes.c_int32 * max(n, 1))()
    scales = (ctypes.c_float * max(n, 1))()
    divs = (ctypes.c_float * max(n, 1))()
    values = (ctypes.c_void_p * max(n, 1))()
    for i, t in enumerate(losses):
      pl = getattr(t, '_er_partials', None)
      if pl is not None:
        src[i], parts[i], scales[i], divs[i], values[i] = pl[0].data_ptr(), pl[0].numel(), float(pl[1]), float(pl[2]), t.data_ptr()
      else:
        src[i], parts[i], scales[i], divs[i], values[i] = t.data_ptr(), 0, 1.0, 1.0, None
    arr = (TailJob * max(len(jobs), 1))()
    for q, (partial, d, n_cols) in zip(arr, jobs):
      assert partial.dim() == 2 and partial.stride(1) == 1 and d.is_contiguous() and d.numel() == n_cols
      q.partial, q.dst, q.n_parts, q.n_cols, q.ld = partial.data_ptr(), d.data_ptr(), partial.shape[0], int(n_cols), partial.stride(0)
    n_part = 0 if emb_partials is None else emb_partials.numel()
    n_dense = 0 if dense_partials is None else dense_partials.numel()
    if defer:
      assert self._deferred_loss_tail is None, 'the previous deferred loss tail was never run'
      vp = ctypes.c_void_p
      job = LossTailJob(_p(emb_partials), n_part, float(emb_scale), _p(dense_partials), n_dense,
                        ctypes.cast(src, vp), ctypes.cast(dst, vp), ctypes.cast(parts, vp), ctypes.cast(scales, vp),
                        ctypes.cast(divs, vp), ctypes.cast(values, vp), n, ctypes.cast(arr, vp), len(jobs),
                        _p(reg_out), _p(total_out))
      # (the record points into the ctypes arrays and the tensors: both stay alive with it)
      self._deferred_loss_tail = (job, (src, dst, parts, scales, divs, values, arr, emb_partials, dense_partials, list(losses),
                                        list(reports), reg_out, total_out, list(jobs)))
      return
    self.ck.er_loss_tail(_p(emb_partials), n_part, emb_scale, _p(dense_partials),
                         n_dense, src, dst, parts, scales, divs, values, n, arr,
                         len(jobs), _p(reg_out), _p(total_out), _stream())

  # the deferred loss tail is per THREAD: the embedding-parallel tests run their ranks as threads over this one backend
  _tail_tls = threading.local()

  @property
  def _deferred_loss_tail(self):
    return getattr(HipBackend._tail_tls, 'pending', None)

  @_deferred_loss_tail.setter
  def _deferred_loss_tail(self, value):
    HipBackend._tail_tls.pending = value

  def discard_loss_tail(self):
    """Forget a deferred loss tail nobody ran (the step that queued it raised before its tail): called at the start of
    every step."""
    self._deferred_loss_tail = None

  def flush_loss_tail(self):
    """Run a deferred loss tail on its own (a step whose tail did not take it)."""
    pending = self._deferred_loss_tail
    if pending is None:
      return
    self._deferred_loss_tail = None
    j = pending[0]
    self.ck.er_loss_tail(j.emb_partials, j.n_partials, j.emb_scale, j.dense_partials, j.n_dense, j.losses,
                         j.report, j.loss_parts, j.loss_scales, j.loss_divs, j.loss_values, j.n_losses, j.jobs,
                         j.n_jobs, j.reg_out, j.total_out, _stream())

  def l2_partials(self, w, coef, partials):
    """partials[b] = sum over weights [256 b, 256 b + 256) of 0.5 * coef * w^2 (what dense_opt_step(l2_partials=) keeps
    current from then on)."""
    assert partials.numel() == (w.numel() + 255) // 256
    self.ck.er_l2_partials(_p(w), _p(coef), w.numel(), _p(partials), _stream())

  def reduce_sum(self, partials, scale, out, accumulate=False):
    self.ck.er_reduce_sum(_p(partials), partials.numel(), scale, _p(out), int(accumulate),
                          _stream())

  def l2_loss(self, w, coef, out, accumulate=False):
    self.ck.er_l2_loss(_p(w), _p(coef), w.numel(), _p(out), int(accumulate), _stream())

  # -- K11 MMoE
  def mmoe_mix_fwd(self, experts, gate_logits):
    E, B, H = experts.shape
    T = gate_logits.shape[0]
    gates = torch.empty_like(gate_logits)
    out = torch.empty(T, B, H, dtype=torch.float32, device=experts.device)
    self.ck.er_mmoe_mix_fwd(_p(_f32c(experts)), _p(_f32c(gate_logits)), T, E, B, H, _p(gates), _p(out),
                            _stream())
    return out, gates

  def mmoe_mix_bwd(self, experts, gates, dout):
    E, B, H = experts.shape
    T = gates.shape[0]
    dexperts = torch.empty_like(experts)
    dlogits = torch.empty_like(gates)
    self.ck.er_mmoe_mix_bwd(_p(experts), _p(gates), _p(_f32c(dout)), T, E, B, H, _p(dexperts), _p(dlogits),
                            _stream())
    return dexperts, dlogits

  def hyper_select(self, table, counter, out, history=None, history_index=HYPER_LR_T):
    """history: fp32 [2 * capacity]: value of step s at [s], the running maximum of the values at [capacity + s]."""
    n_slots = table.shape[0]
    cap = 0 if history is None else history.numel() // 2
    self.ck.er_hyper_select(_p(table), _p(counter), n_slots, table[0].numel(), _p(out), _p(history),
                            cap, history_index, _stream())

  def step_prologue(self, table, counter, out, history=None, zero=None, history_index=HYPER_LR_T, decay_tables=None,
                    hash_job=None):
    """hyper_select + zeroing of `zero` (the flat gradient buffer) in one launch.  decay_tables (decay_tables_create):
    the same launch appends the step's entry to the closed-form replay's per-step table.  hash_job = (bytes, offsets,
    n_per_col, num_buckets, drop_empty, out) (hash_bucket_fast's arguments): the batch's id strings are hashed by further
    workgroups of the same launch."""
    n_slots = table.shape[0]
    cap = 0 if history is None else history.numel() // 2
    nz = 0 if zero is None else zero.numel()
    assert zero is None or (zero.dtype == torch.float32 and zero.is_contiguous())
    hb = ho = hk = hout = None
    hn, hpc, hdrop = 0, 1, 0
    if hash_job is not None:
      hb, ho, hpc, hk, hdrop, hout = hash_job
      hn = ho.numel() - 1
      assert hout.dtype == torch.int64 and hout.numel() >= hn
    self.ck.er_step_prologue_hash(_p(table), _p(counter), n_slots, table[0].numel(), _p(out), _p(history),
                                  cap, history_index, _p(zero), nz,
                                  decay_tables['handle'] if decay_tables else None, _p(hb), _p(ho), hn,
                                  int(hpc), _p(hk), int(hdrop), _p(hout), _stream())

  # -- closed-form replay of TF-Adam's decay-only steps (csrc/er_decay.h)
  def decay_tables_create(self, lr_hist, step_counter, beta1, beta2):
    """The tables of the closed-form replay for the history buffer `lr_hist` ([2 * capacity]) - or None when the
    betas are outside its range (the groups then keep the exact step-by-step replay)."""
    if self.lib.er_decay_tables_supported(beta1, beta2) <= 0:
      return None
    cap = lr_hist.numel() // 2
    nbytes = int(self.lib.er_decay_tables_bytes(cap))
    buf = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=lr_hist.device)
    handle = ctypes.c_void_p()
    self.ck.er_decay_tables_create(_p(buf), cap, _p(lr_hist), _p(step_counter),
                                   beta1, beta2, ctypes.byref(handle))
    return {'handle': handle, 'buffer': buf, 'lr_hist': lr_hist, 'step_counter': step_counter,
            'betas': (float(beta1), float(beta2))}

  def decay_tables_destroy(self, tabs):
    if tabs is not None and tabs.get('handle') is not None:
      self.lib.er_decay_tables_destroy(tabs['handle'])
      tabs['handle'] = None

  def emb_group_set_decay_tables(self, group, tabs):
    self.ck.er_emb_group_set_decay_tables(group['handle'], tabs['handle'] if tabs else None)
    group['decay_tables'] = tabs

  # -- TF-exact Adam without the sweep (lazy dense decay)
  def emb_group_enable_lazy_decay(self, group, last_step, lr_hist, step_counter):
    """lr_hist: the [2 * capacity] history buffer of hyper_select (values | running maxima)."""
    assert last_step.dtype == torch.int32 and lr_hist.dtype == torch.float32 and step_counter.dtype == torch.int64
    self.ck.er_emb_group_enable_lazy_decay(group['handle'], _p(last_step), _p(lr_hist), _p(step_counter))
    cap = lr_hist.numel() // 2
    if True:  # (the absorbed regime of the replay)
      self.ck.er_emb_group_set_lr_max(group['handle'], _p(lr_hist[cap:]))
    group['last_step'], group['lr_hist'], group['step_counter'] = last_step, lr_hist, step_counter
    self._set_row_pitch(group)

  def emb_flush_window(self, groups, n_windows, hyper, lag=0, max_blocks=0):
    """Rolling flush: this step's window (step mod n_windows) of up to 4 table groups, one launch.  lag 1: the
    variant that runs concurrently with the step (after its catch-up, on another stream)."""
    n = len(groups)
    gh = (ctypes.c_void_p * n)(*[g['handle'] for g in groups])
    self.ck.er_emb_flush_window(gh, n, int(n_windows), int(lag), int(max_blocks), _p(hyper), _stream())

  def emb_catch_up(self, group, unique_keys, n_unique, hyper):
    self.ck.er_emb_catch_up(group['handle'], _p(unique_keys), _p(n_unique), _p(hyper), _stream())

  def emb_catch_up_multi(self, groups, unique_keys, n_unique, hyper):
    """er_emb_catch_up for several table groups in one launch (same results)."""
    n = len(groups)
    gh = (ctypes.c_void_p * n)(*[g['handle'] for g in groups])
    uk = (ctypes.c_void_p * n)(*[t.data_ptr() for t in unique_keys])
    nu = (ctypes.c_void_p * n)(*[t.data_ptr() for t in n_unique])
    self.ck.er_emb_catch_up_multi(gh, uk, nu, n, _p(hyper), _stream())

  def emb_bwd_update_multi(self, groups, opt_kind, hyper):
    """er_emb_bwd_update for several table groups: one tile launch and one fix launch for all (same results)."""
    n = len(groups)
    gh = (ctypes.c_void_p * n)(*[g['handle'] for g in groups])
    self.ck.er_emb_bwd_update_multi(gh, n, opt_kind, _p(hyper), _stream())

  # the end of an embedding-parallel step - owner fix | replicated apply | dense optimizer - as one launch - A/B switch
  ep_update_tail = os.environ.get('EASYREC_AMD_EP_UPDATE_TAIL', '1') != '0'

  def emb_owner_update_tail(self, groups, opt_kind, hyper, tables, dense_opt):
    """er_emb_owner_update_tail: emb_bwd_update_multi(groups) whose fix launch also carries emb_dense_apply(tables) and
    dense_opt_step(*dense_opt) (dense_opt = (w, m, v, grad, l2coef, kind, hyper, l2_partials)); <= 4 groups, <= 4 tables."""
    n, nt = len(groups), len(tables)
    gh = (ctypes.c_void_p * n)(*[g['handle'] for g in groups])
    descs = (DenseApplyDesc * max(nt, 1))()
    for i, (var, m, v, dense) in enumerate(tables):
      assert var.stride(1) == 1 and dense.stride(1) == 1 and dense.shape[0] == var.shape[0]
      assert all(t is None or t.stride() == var.stride() for t in (m, v))
      descs[i] = DenseApplyDesc(var.data_ptr(), None if m is None else m.data_ptr(), None if v is None else v.data_ptr(),
                                dense.data_ptr(), dense.stride(0), var.shape[1], var.shape[0], var.stride(0))
    w, m, v, grad, l2coef, kind, hyp, l2p = dense_opt
    oj = DenseOptJob(_p(w), _p(m), _p(v), _p(grad), _p(l2coef), w.numel(), int(kind), _p(hyp), _p(l2p))
    self.ck.er_emb_owner_update_tail(gh, n, opt_kind, _p(hyper), descs if nt else None, nt,
                                     ctypes.byref(oj), _stream())
    st = self._bf16_state_of(w)
    if st is not None:
      st.refresh()  # the weights' bf16 shadows follow the masters (one launch)

  def emb_flush_decay(self, group, hyper):
    self.ck.er_emb_flush_decay(group['handle'], _p(hyper), _stream())

  # -- gradient clipping by global norm (compat/optimizers.py:365-376, 453-481)
  def gradsq_rows(self, x, cols, weight, acc, accumulate, counts=None, seg_stride=None):
    """acc[0] (+)= weight * sum of x[r, :cols]^2 over the valid rows: all of them, or (counts int32 [n_seg]) the rows
    with (r % seg_stride) < counts[r // seg_stride]; seg_stride None = the whole buffer is one segment."""
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == torch.float32 and acc.dtype == torch.float32
    rows = x.shape[0]
    n_seg = 0 if counts is None else counts.numel()
    assert counts is None or counts.dtype == torch.int32
    stride = rows if seg_stride is None else int(seg_stride)
    self.ck.er_gradsq_rows(_p(x), rows, int(cols), x.stride(0), _p(counts), n_seg, max(stride, 1), weight,
                           _p(acc), accumulate, _stream())

  def gradsq_dense(self, w, grad, l2coef, hyper, acc, accumulate=False):
    """acc[0] (+)= sum (hyper.grad_scale * grad + l2coef * w)^2: the dense gradient as er_dense_opt_step sees it."""
    self.ck.er_gradsq_dense(_p(w), _p(grad), _p(l2coef), w.numel(), _p(hyper), _p(acc),
                            accumulate, _stream())

  def clip_scale(self, normsq, clip_norm, records, norm_out=None):
    """records [n, HYPER_FLOATS] (device): records[:, HYPER_CLIP] = clip_norm * min(1 / norm, 1 / clip_norm)."""
    assert records.dim() == 2 and records.shape[1] == HYPER_FLOATS and records.is_contiguous()
    self.ck.er_clip_scale(_p(normsq), clip_norm, _p(records), records.shape[0],
                          _p(norm_out), _stream())

  def emb_apply_unique(self, group, keys, grads, n_unique, opt_kind, hyper):
    """The row-wise optimizer of emb_bwd_update on ready-made de-duplicated row sums (emb_bwd_reduce[_routed])."""
    assert keys.dtype == torch.int32 and n_unique.dtype == torch.int32 and grads.dim() == 2 and grads.stride(1) == 1
    self.ck.er_emb_apply_unique(group['handle'], _p(keys), _p(grads), grads.stride(0),
                                _p(n_unique), opt_kind, _p(hyper), _stream())

  # -- dense optimizer
  def dense_opt_step(self, w, m, v, grad, l2coef, opt_kind, hyper, l2_partials=None):
    """l2_partials: left holding the per-256-weight sums of 0.5 * l2coef * w_new^2 (the next step's kernel-L2 loss)."""
    self.ck.er_dense_opt_step_l2(_p(w), _p(m), _p(v), _p(grad), _p(l2coef), w.numel(),
                                 opt_kind, _p(hyper), _p(l2_partials), _stream())
    st = self._bf16_state_of(w)
    if st is not None:
      st.refresh()  # the weights' bf16 shadows follow the masters (one launch)


_BACKEND = None


def hip():
  """The kernel backend used by every layer of this package."""
  global _BACKEND
  if _BACKEND is None:
    _BACKEND = HipBackend()
  return _BACKEND


# ---------------------------------------------------------------------------------------------
# autograd glue: dense activations flow through torch.autograd; each Function is one fused kernel
# forward and one backward.
# ---------------------------------------------------------------------------------------------
def _take_pending_bn(be, x, src, w, bf16):
  """x may be the output of a layer whose BatchNorm apply was deferred to its consumer (LinearBNActFn / DINFirstLayerFn with
  defer_apply): -> the pending record when the apply can run inside the staging of the contraction x . w
  (HipBackend.gemm_bn_a), else None - after running the apply as the launch of its own it would have been."""
  pin = src.pending if isinstance(src, BnSource) else None
  if pin is None:
    return None
  src.pending = None
  if x.dim() == 2 and x.stride(-1) == 1 and not bf16 and getattr(be, 'bn_in_staging', False) and \
      pin['y'].data_ptr() == x.data_ptr() and pin['y'].shape == x.shape and be.bn_a_ok(pin, w):
    return pin
  be.bn_apply_pending(pin)
  return None


class LinearFn(torch.autograd.Function):
  """y = x . W (+ b): tf.layers.dense without activation (reference layers/dnn.py:57-62).  Forward and both
  gradients are hand-written MFMA GEMMs (er_gemm_*).  The weight/bias gradients are accumulated straight
  into the variables' slices of the flat gradient buffer (`w_grad`, `b_grad`; zeroed once per step by
  VarStore.zero_grad), so autograd issues no per-variable add kernels; when no buffer is given they are
  returned the normal way."""

  @staticmethod
  def forward(ctx, x, w, b, w_grad, b_grad, bf16, src=None, sink=None):
    be = hip()
    pin = _take_pending_bn(be, x, src, w, bf16)
    x2 = x if x.stride(-1) == 1 else x.contiguous()
    y = be.gemm_bn_a(pin, w, b) if pin is not None else be.gemm(GEMM_NN, x2, w, bias=b, bf16=bf16)
    ctx.save_for_backward(x2, w)
    ctx.has_bias = b is not None
    ctx.w_grad, ctx.b_grad, ctx.bf16 = w_grad, b_grad, bf16
    ctx.sink = be.wgrad_sink()
    ctx.src = src if (src is not None and x2 is x and _bn_bwd_fusable(be, bf16) and src.fused) else None
    ctx.gsink = sink if x2 is x else None
    # (x's other consumers may share its gradient buffer: grad_slot)
    ctx.slots = grad_slots_of_step() if (x2 is x and x.dim() == 2 and x.is_contiguous()) else None
    return y

  @staticmethod
  def backward(ctx, dy):
    be = hip()
    x, w = ctx.saved_tensors
    dy = dy if dy.stride(-1) == 1 and dy.dim() == 2 else dy.contiguous()
    dx = dw = db = None
    if ctx.needs_input_grad[0]:
      dx = _dgrad(be, dy, w, ctx.src, ctx.bf16, ctx.gsink, x, ctx.slots)
    with_bias = False
    if ctx.needs_input_grad[1]:
      # (a tall projection onto <= 4 columns: weight AND bias gradient from one pass over dy - HipBackend.wgrad_tall_narrow)
      with_bias = bool(ctx.has_bias and ctx.needs_input_grad[2] and ctx.b_grad is not None and ctx.w_grad is not None and
                       not ctx.bf16 and hasattr(be, 'wgrad_tall_narrow_ok') and be.wgrad_tall_narrow_ok(x, dy) and
                       ctx.w_grad.stride(-1) == 1 and ctx.b_grad.is_contiguous())
      if with_bias:
        be.wgrad_tall_narrow(x, dy, ctx.w_grad, accumulate=True, bias_grad=ctx.b_grad)
      else:
        dw = _wgrad(be, x, dy, ctx.w_grad, ctx.bf16, ctx.sink)
    if ctx.has_bias and ctx.needs_input_grad[2] and not with_bias:
      if ctx.b_grad is not None:
        be.colsum(dy, out=ctx.b_grad, accumulate=True)  # straight into the flat gradient buffer
      else:
        db = be.colsum(dy)
    return dx, dw, db, None, None, None, None, None


class HeadState(object):
  """A rank model's `output` projection (dense(K -> 1)) whose logits have not been computed yet: layers/dnn.py dense(head=True)
  registers it; builders/loss_builder.py either runs the fused head launch on it (HipBackend.head_sigmoid_ce: logits, loss,
  and the projection's whole backward) or materialises the logits with an ordinary GEMM (materialize_head)."""
  __slots__ = ('x', 'w', 'b', 'w_grad', 'b_grad', 'src', 'logits', 'state', 'dx', 'dz', 'bf16')

  def __init__(self, x, w, b, w_grad, b_grad, src, logits, bf16):
    self.x, self.w, self.b, self.w_grad, self.b_grad, self.src, self.logits, self.bf16 = x, w, b, w_grad, b_grad, src, logits, bf16
    self.state, self.dx, self.dz = 'pending', None, None

  @property
  def fusable(self):
    K = self.x.shape[1]
    return (self.state == 'pending' and self.w_grad is not None and (self.b is None or self.b_grad is not None) and
            K % 4 == 0 and K <= 256 and self.x.stride(0) % 4 == 0 and self.x.data_ptr() % 16 == 0 and self.w.data_ptr() % 16 == 0)


def pending_head(pred):
  """The HeadState whose logits buffer `pred` views (same storage start), while it is still pending; else None."""
  from easyrec_amd.core import context
  stack = context._stack()
  heads = getattr(stack[-1], 'heads', None) if stack else None
  if not heads:
    return None
  st = heads.get(pred.data_ptr())
  return st if (st is not None and st.state == 'pending' and pred.numel() == st.logits.numel()) else None


def materialize_head(st):
  """logits = x . w + b by the ordinary GEMM (the loss is not the fused sigmoid cross entropy)."""
  if st.state == 'pending':
    hip().gemm(GEMM_NN, st.x, st.w.detach(), out=st.logits, bias=None if st.b is None else st.b.detach(), bf16=st.bf16)
    st.state = 'materialized'


def materialize_pending_heads():
  from easyrec_amd.core import context
  stack = context._stack()
  for st in list(getattr(stack[-1], 'heads', {}).values()) if stack else []:
    materialize_head(st)


class HeadFn(torch.autograd.Function):
  """LinearFn for the logit head of a rank model (units = 1): the forward only RESERVES the logits; the loss builder fills
  them - together with the loss and this layer's complete backward (HeadState / HipBackend.head_sigmoid_ce) - or falls back
  to the GEMMs of LinearFn."""

  @staticmethod
  def forward(ctx, x, w, b, w_grad, b_grad, bf16, src, heads):
    x2 = x if x.stride(-1) == 1 else x.contiguous()
    logits = torch.empty(x2.shape[0], 1, dtype=torch.float32, device=x2.device)
    be = hip()
    # (the head launch itself is fp32 arithmetic on fp32 activations, whatever the dense dtype)
    fused = src is not None and x2 is x and src.fused and _bn_bwd_fusable(be, bf16)
    # (the state keeps a DETACHED alias of the logits: they are written after this forward returned, outside autograd's view)
    st = HeadState(x2, w.detach(), None if b is None else b.detach(), w_grad, b_grad, src if fused else None, logits.detach(), bf16)
    heads[logits.data_ptr()] = st
    ctx.st = st
    ctx.save_for_backward(x2, w)
    ctx.has_bias = b is not None
    ctx.sink = be.wgrad_sink()
    return logits

  @staticmethod
  def backward(ctx, dy):
    be = hip()
    st = ctx.st
    x, w = ctx.saved_tensors
    if st.state == 'fused':
      # the loss launch already produced dx and queued dW / db for the loss tail: dy must be the gradient it computed
      # (autograd may hand over a copy of the seed; build_loss_graph seeds exactly one gradient per logits tensor)
      assert dy.numel() == st.dz.numel()
      return st.dx, None, None, None, None, None, None, None
    assert st.state == 'materialized', 'the logits of a rank model\'s head were never computed (kernels.materialize_head)'
    dy = dy if dy.stride(-1) == 1 and dy.dim() == 2 else dy.contiguous()
    dx = dw = db = None
    if ctx.needs_input_grad[0]:
      dx = _dgrad(be, dy, w, st.src, st.bf16, None)
    if ctx.needs_input_grad[1]:
      dw = _wgrad(be, x, dy, st.w_grad, st.bf16, ctx.sink)
    if ctx.has_bias and ctx.needs_input_grad[2]:
      if st.b_grad is not None:
        be.colsum(dy, out=st.b_grad, accumulate=True)
      else:
        db = be.colsum(dy)
    return dx, dw, db, None, None, None, None, None


def _bn_bwd_fusable(be, bf16):
  """May a consumer's input-gradient contraction emit the producer's BatchNorm-backward column sums?  fp32: er_gemm_f32_bn_bwd;
  bf16: the same epilogue of er_gemm_bf16_nt_epi (bf16 operands in HBM)."""
  if not getattr(be, 'fused_bn_bwd', False):
    return False
  return (not bf16) or bool(getattr(be, 'bf16_nt', False) and getattr(be, 'bf16_epilogues', False))


def _wgrad(be, x, dz, w_grad, bf16, sink):
  """dW = x^T . dz: queued for the grouped launch (accumulating into w_grad, a slice of the flat gradient buffer), else
  launched here.  Returns dW only without w_grad."""
  if w_grad is not None:
    if not bf16 and hasattr(be, 'wgrad_tall_narrow_ok') and be.wgrad_tall_narrow_ok(x, dz) and w_grad.stride(-1) == 1:
      be.wgrad_tall_narrow(x, dz, w_grad, accumulate=True)  # (a [rows, 1] operand would stall the grouped launch: see there)
    elif not sink.put(x, dz, w_grad, bf16):
      be.gemm(GEMM_TN, x, dz, out=w_grad, accumulate=True, bf16=bf16)
    return None
  return be.gemm(GEMM_TN, x, dz, bf16=bf16)


def _dgrad(be, dz, w, src, bf16, sink=None, x=None, slots=None):
  """dx = dz . W^T; when the input was the output of a fused dense + BatchNorm layer (src), the GEMM's epilogue also
  leaves that layer's BatchNorm-backward column sums in src.partial; when it was an embedding group output (sink),
  the GEMM accumulates straight into the group's gradient buffer and nothing is returned to autograd."""
  if sink is not None and sink.covers(0, w.shape[0]):
    dst, acc = sink.target(0, w.shape[0])
    be.gemm(GEMM_NT, dz, w, out=dst, accumulate=acc, bf16=bf16)
    sink.done()
    return None
  if src is None:
    slot = grad_slot(slots, x) if (x is not None and slots is not None) else None
    if slot is not None and not slot[2]:
      # another consumer of x already started its gradient (a cross layer's epilogue): this GEMM accumulates into it
      be.gemm(GEMM_NT, dz, w, out=slot[0], accumulate=True, bf16=bf16)
      return None
    if slot is not None:
      return be.gemm(GEMM_NT, dz, w, out=slot[0], bf16=bf16)
    return be.gemm(GEMM_NT, dz, w, bf16=bf16)
  M, N = dz.shape[0], w.shape[0]
  if isinstance(src, BnColsView):
    inner = src.src
    n_src = inner.y.shape[1]
    partial = torch.empty(be.gemm_row_tiles(M) * n_src * 2, dtype=torch.float32, device=dz.device)
    dx = be.gemm_bn_bwd(GEMM_NT, dz, w, inner, partial, col0=src.col0, **({'bf16': True} if bf16 else {}))
    if dx is None:  # (bf16: shapes the epilogue does not take)
      return be.gemm(GEMM_NT, dz, w, bf16=bf16)
    inner.partial, inner.dx_ptr = partial, dx.data_ptr() + 4 * src.col0  # (what the block's view of dx starts at)
    return dx
  partial = torch.empty(be.gemm_row_tiles(M) * N * 2, dtype=torch.float32, device=dz.device)
  dx = be.gemm_bn_bwd(GEMM_NT, dz, w, src, partial, **({'bf16': True} if bf16 else {}))
  if dx is None:
    return be.gemm(GEMM_NT, dz, w, bf16=bf16)
  src.partial, src.dx_ptr = partial, dx.data_ptr()
  return dx


class LinearBNActFn(torch.autograd.Function):
  """dense (+ bias) -> BatchNorm(train) -> activation of one DNN layer (reference layers/dnn.py:57-79) as TWO
  launches forward: the MFMA GEMM, whose epilogue adds the bias and emits per-row-tile column statistics, and
  one fused finalize + normalise + ReLU kernel.  Backward: column sums, fused finalize + dz, then the two
  gradient GEMMs; parameter gradients accumulate straight into the flat gradient buffer (`grad_bufs` =
  (kernel.grad, gamma.grad, beta.grad)).  Under BatchNorm d(loss)/d(bias) == 0, so the bias gets none."""

  @staticmethod
  def forward(ctx, x, w, b, gamma, beta, moving_mean, moving_var, eps, momentum, act, bf16, grad_bufs, src=None,
              sink=None, defer_apply=False):
    be = hip()
    pin = _take_pending_bn(be, x, src, w, bf16)
    x2 = x if x.stride(-1) == 1 else x.contiguous()
    M, N = x2.shape[0], w.shape[1]
    chunks = be.gemm_row_tiles(M)
    stats = torch.empty(chunks * N * 3, dtype=torch.float32, device=x2.device)
    if pin is not None:
      z = be.gemm_bn_a(pin, w, b, col_stats=stats)
    else:
      z = be.gemm(GEMM_NN, x2, w, bias=b, bf16=bf16, col_stats=stats)
    # (bf16: the BatchNorm launch writes the bf16 copy the next contraction reads; its backward the one the dgrad reads)
    ctx.b16 = be._bf16_state_of(w) if (bf16 and getattr(be, 'bf16_nt', False) and getattr(be, 'bf16_epilogues', False)) else None
    # defer_apply: the caller's NEXT op on y is the one consumer that runs this layer's BatchNorm finalize + apply inside its
    # own launch (DeepFM: WideFmConcatFn).  Until then y / mean / invstd are unwritten buffers.
    pend = None
    # (defer_apply == 'staging': the consumer is the next layer's LinearBNActFn - a tall layer, HipBackend.bn_in_staging)
    if defer_apply and not bf16 and _bn_bwd_fusable(be, bf16) and z.is_contiguous() and \
        getattr(be, 'bn_in_staging' if defer_apply == 'staging' else 'defer_bn_apply', False):
      y = torch.empty_like(z)
      mean = torch.empty(N, dtype=torch.float32, device=z.device)
      invstd = torch.empty(N, dtype=torch.float32, device=z.device)
      pend = dict(z=z, stats=stats, chunks=chunks, gamma=gamma.detach(), beta=beta.detach(), eps=eps, momentum=momentum,
                  moving_mean=moving_mean, moving_var=moving_var, act=act, y=y, mean=mean, invstd=invstd)
    else:
      y, mean, invstd = be.bn_apply_from_stats(z, None, stats, chunks, gamma, beta, eps, momentum, moving_mean,
                                               moving_var, act, **({'bf16_state': ctx.b16} if ctx.b16 is not None else {}))
    ctx.save_for_backward(x2, w, gamma, beta, z, y, mean, invstd)
    ctx.act, ctx.bf16, ctx.grad_bufs = act, bf16, grad_bufs
    ctx.sink = be.wgrad_sink()
    fused = _bn_bwd_fusable(be, bf16)
    ctx.src = src if (src is not None and x2 is x and fused and src.fused) else None
    ctx.gsink = sink if x2 is x else None
    gb = None if grad_bufs is None else (grad_bufs[1], grad_bufs[2])
    # (z already carries the bias)
    ctx.own = BnSource(z, None, y, mean, invstd, act, gamma, gb, beta=beta, fused=fused) if fused else None
    if pend is not None:
      ctx.own.pending = pend
    _bn_tls.last = ctx.own
    return y

  @staticmethod
  def backward(ctx, dy):
    be = hip()
    x, w, gamma, beta, z, y, mean, invstd = ctx.saved_tensors
    assert ctx.own is None or ctx.own.pending is None, 'a deferred BatchNorm apply was never run (kernels.finish_pending_bn)'
    wg, gg, betag = ctx.grad_bufs if ctx.grad_bufs is not None else (None, None, None)
    direct = gg is not None and betag is not None
    # (a column block of a wider gradient - ConcatFn's backward - is read in place by the BatchNorm backward)
    dyc = dy if (dy.dim() == 2 and dy.stride(1) == 1) else dy.contiguous()
    own, partial = ctx.own, None
    dgamma = dbeta = None
    if own is not None:
      # the consumer's dgrad GEMM already reduced the column sums, provided dy is exactly its output
      if own.partial is not None and dyc.data_ptr() == own.dx_ptr:
        partial = own.partial
      own.partial = None
    dz, _, dgamma, dbeta = be.bn_act_bwd(z, None, gamma, y, mean, invstd, dyc, 1, ctx.act, False, True,
                                         into=(None, gg, betag) if direct else None, partial=partial, beta=beta,
                                         **({'bf16_state': ctx.b16} if (ctx.b16 is not None and ctx.needs_input_grad[0]) else {}))
    dx = dw = None
    if ctx.needs_input_grad[0]:
      dx = _dgrad(be, dz, w, ctx.src, ctx.bf16, ctx.gsink)
    if ctx.needs_input_grad[1]:
      dw = _wgrad(be, x, dz, wg, ctx.bf16, ctx.sink)
    return dx, dw, None, dgamma, dbeta, None, None, None, None, None, None, None, None, None, None


def finish_pending_bn(t):
  """Run the deferred BatchNorm finalize + apply behind tensor t (LinearBNActFn(defer_apply=True)) as a launch of its own, if
  it is still pending: what a consumer that cannot fold it calls before it reads t."""
  src = bn_source_of(t)
  if src is not None and src.pending is not None:
    hip().bn_apply_pending(src.pending)
    src.pending = None


class GroupedLinearFn(torch.autograd.Function):
  """The same-depth dense layers z_e = x_e . W_e (+ b_e) of E PARALLEL stacks - MMoE's experts, the task towers, the
  gates (reference layers/mmoe.py:62-83, model/multi_task_model.py:33-100, which issue them one after the other) - as ONE
  grouped launch forward (er_gemm_grouped_f32: bias in the epilogue, optionally the column statistics a BatchNorm needs)
  and ONE grouped launch for the input gradients; weight gradients join the step's grouped weight-gradient launch, bias
  gradients are column sums into the flat gradient buffer.  Layers that read the SAME input (the first depth of MMoE:
  every expert and gate reads the shared features) accumulate their input gradients into one buffer - or straight into the
  embedding group's gradient buffer (`sinks`) - one GEMM after the other, as the sequential form does.
  apply(E, stats_mask, sinks, x_0..x_{E-1}, W_0.., b_0.. (None ok)) -> (z_0 .. z_{E-1}, stats_0 .. stats_{E-1}) (stats_e:
  an empty tensor unless stats_mask[e])."""

  @staticmethod
  def forward(ctx, E, stats_mask, sinks, srcs, *args):
    be = hip()
    xs, ws, bs = args[:E], args[E:2 * E], args[2 * E:3 * E]
    # fzs[e]: None, or dict(bias, gamma, beta, moving_mean, moving_var, eps, act) - layer e's output also goes through the frozen
    # BatchNorm + activation in the launch's epilogue; the outputs then carry (y_e, save_e = [mean | invstd]) behind the statistics
    fzs = args[3 * E] if len(args) > 3 * E else None
    ctx.has_fzs = len(args) > 3 * E
    ctx.gsinks = [sk if (sk is not None and x.stride(-1) == 1) else None for sk, x in zip(sinks, xs)]
    # srcs[e]: the BnSource of x_e when it IS the output of a dense + BatchNorm(train) layer: the input-gradient launch
    # then also emits that layer's BatchNorm-backward column sums (er_gemm_problem.bn_*)
    fused = getattr(be, 'fused_bn_bwd', False)
    ctx.srcs = [sc if (fused and sc is not None and sc.fused and x.stride(-1) == 1) else None
                for sc, x in zip(srcs, xs)]
    xs = [x if x.stride(-1) == 1 else x.contiguous() for x in xs]
    zs, stats, problems, pre = [], [], [], []
    for e in range(E):
      M, N = xs[e].shape[0], ws[e].shape[1]
      z = torch.empty(M, N, dtype=torch.float32, device=xs[e].device)
      st = torch.empty(be.gemm_row_tiles(M) * N * 3, dtype=torch.float32, device=z.device) if stats_mask[e] else None
      zs.append(z)
      stats.append(st if st is not None else torch.empty(0, device=z.device))
      fz = None
      if fzs is not None and fzs[e] is not None:
        assert bs[e] is None and st is None
        fz = dict(fzs[e], y=torch.empty_like(z), save=torch.empty(2, N, dtype=torch.float32, device=z.device))
        pre += [fz['y'], fz['save']]
      elif fzs is not None:
        pre += [torch.empty(0, device=z.device), torch.empty(0, device=z.device)]
      problems.append((xs[e], ws[e].detach(), z, None if bs[e] is None else bs[e].detach(), False, st, None, fz))
    be.gemm_grouped(GEMM_NN, problems)
    ctx.save_for_backward(*xs, *ws)
    ctx.E, ctx.bs = E, bs
    ctx.wgrads = [w.grad if (w.requires_grad and w.grad is not None) else None for w in ws]  # slices of the flat buffer
    ctx.stats_mask = tuple(stats_mask)
    ctx.set_materialize_grads(False)  # (the statistics outputs get no gradient: no zero tensors to be filled for them)
    ctx.sink = be.wgrad_sink()
    ctx.mark_non_differentiable(*stats, *pre)
    return tuple(zs) + tuple(stats) + tuple(pre)

  @staticmethod
  def backward(ctx, *grads):
    be = hip()
    E = ctx.E
    saved = ctx.saved_tensors
    xs, ws = saved[:E], saved[E:2 * E]
    dzs = [None if g is None else (g if (g.dim() == 2 and g.stride(1) == 1) else g.contiguous()) for g in grads[:E]]
    # a stack output left out of the loss (a tower no loss reads) arrives as None (set_materialize_grads(False)): that
    # layer contributes nothing - no input gradient, no weight gradient, no bias gradient - as in the one-by-one form
    dxs = [None] * E
    need = [e for e in range(E) if ctx.needs_input_grad[4 + e] and dzs[e] is not None]
    by_input = {}
    for e in need:
      # readers of ONE input share an accumulation buffer: same storage start AND same shape / strides (a row prefix
      # x[:k] of x shares its base pointer and is a different input)
      by_input.setdefault((xs[e].data_ptr(), tuple(xs[e].shape), tuple(xs[e].stride())), []).append(e)
    solo = [es[0] for es in by_input.values() if len(es) == 1 and ctx.gsinks[es[0]] is None]
    if solo:
      problems = []
      for e in solo:
        dxs[e] = torch.empty_like(xs[e])
        src = ctx.srcs[e]
        if src is None:
          problems.append((dzs[e], ws[e], dxs[e], None, False))
        else:
          M, N = dxs[e].shape
          partial = torch.empty(be.gemm_row_tiles(M) * N * 2, dtype=torch.float32, device=dxs[e].device)
          # (a layer on the moving statistics: the launch also runs its elementwise backward - dxs[e] leaves as dz)
          dz_out = bool(getattr(src, 'frozen', False) and getattr(be, 'frozen_dz_epilogue', False) and not src.dz_done)
          problems.append((dzs[e], ws[e], dxs[e], None, False, None, (src, partial, dz_out)))
          src.partial, src.dx_ptr = partial, dxs[e].data_ptr()
          if dz_out:
            src.dz_done = True
      be.gemm_grouped(GEMM_NT, problems)
    for es in by_input.values():
      if len(es) == 1 and ctx.gsinks[es[0]] is None:
        continue
      sink = ctx.gsinks[es[0]]
      to_sink = sink is not None and sink.covers(0, ws[es[0]].shape[0])  # an embedding group output: into its gradient buffer
      if len(es) > 1 and _CAT_DGRAD and all(dzs[e].stride(1) == 1 for e in es):
        # readers of ONE input (MMoE's first depth: every expert and gate reads the shared features): dx = sum_e dz_e W_e^T
        # is ONE contraction over the layers' output columns laid side by side - the input-sized gradient is written once
        # instead of being read and re-written by a GEMM per layer (8 x 36 MB at B = 8192), for two small concat launches.
        # (The same for the weight gradients - x^T . [dz_1 | dz_2 | ...] as one TN GEMM outside the step's grouped launch,
        # then added to the layers' gradient slices - measured SLOWER: 2.23 against 2.11 ms,
        # profiles/r04_mmoe_cat_wgrad_ab.txt; the grouped launch's split-K scheduling is the better one.)
        dz_cat = be.concat_cols([dzs[e] for e in es])
        w_cat = be.concat_cols([ws[e].detach() for e in es])
        if to_sink:
          _dgrad(be, dz_cat, w_cat, None, False, sink)
        else:
          dxs[es[0]] = be.gemm(GEMM_NT, dz_cat, w_cat)
        continue
      if to_sink:
        for e in es:
          _dgrad(be, dzs[e], ws[e], None, False, sink)
        continue
      acc = torch.empty_like(xs[es[0]])  # readers of one input: one buffer, accumulated GEMM by GEMM; the sum is returned
      for j, e in enumerate(es):         # for the first of them, the others contribute nothing more
        be.gemm(GEMM_NT, dzs[e], ws[e], out=acc, accumulate=j > 0)
      dxs[es[0]] = acc
    dws, dbs = [None] * E, [None] * E
    narrow = []  # the bias gradients of narrow layers (tower heads [B, 1], gates [B, experts]): ONE launch for all of them
    for e in range(E):
      if dzs[e] is None:
        continue
      if ctx.needs_input_grad[4 + E + e]:
        dws[e] = _wgrad(be, xs[e], dzs[e], ctx.wgrads[e], False, ctx.sink)
      b = ctx.bs[e]
      # (a layer whose output feeds BatchNorm on batch statistics - stats_mask - has a bias gradient of exactly zero)
      if b is not None and not ctx.stats_mask[e] and ctx.needs_input_grad[4 + 2 * E + e]:
        if b.grad is not None:
          if hasattr(be, 'colsum_narrow_multi') and be.colsum_is_narrow(dzs[e]) and b.grad.is_contiguous():
            narrow.append((dzs[e], b.grad))
          else:
            be.colsum(dzs[e], out=b.grad, accumulate=True)
        else:
          dbs[e] = be.colsum(dzs[e])
    if len(narrow) == 1:
      be.colsum(narrow[0][0], out=narrow[0][1], accumulate=True)
    elif narrow:
      be.colsum_narrow_multi(narrow, accumulate=True)
    return (None, None, None, None) + tuple(dxs) + tuple(dws) + tuple(dbs) + ((None,) if ctx.has_fzs else ())


class BNFromStatsFn(torch.autograd.Function):
  """BatchNorm(train) + activation of a GEMM output whose per-row-tile column statistics its launch already produced
  (GroupedLinearFn): er_bn_apply_from_stats forward, er_bn_act_bwd backward (parameter gradients into the flat buffer)."""

  @staticmethod
  def forward(ctx, z, stats, gamma, beta, moving_mean, moving_var, eps, momentum, act, grad_bufs):
    be = hip()
    y, mean, invstd = be.bn_apply_from_stats(z, None, stats, be.gemm_row_tiles(z.shape[0]), gamma, beta, eps, momentum,
                                             moving_mean, moving_var, act)
    ctx.save_for_backward(z, gamma, y, mean, invstd)
    ctx.act, ctx.grad_bufs = act, grad_bufs
    ctx.beta = None if beta is None else beta.detach()  # (read by the backward's mask recomputation only)
    fused = getattr(be, 'fused_bn_bwd', False)
    ctx.own = BnSource(z, None, y, mean, invstd, act, gamma, grad_bufs, beta=beta, fused=fused) if fused else None
    _bn_tls.last = ctx.own
    return y

  @staticmethod
  def backward(ctx, dy):
    be = hip()
    z, gamma, y, mean, invstd = ctx.saved_tensors
    gg, betag = ctx.grad_bufs if ctx.grad_bufs is not None else (None, None)
    direct = gg is not None and betag is not None
    dyc = dy if (dy.dim() == 2 and dy.stride(1) == 1) else dy.contiguous()
    own, partial = ctx.own, None
    if own is not None:
      # the consumer's input-gradient launch already reduced the column sums, provided dy is exactly its output
      if own.partial is not None and dyc.data_ptr() == own.dx_ptr:
        partial = own.partial
      own.partial = None
    dz, _, dgamma, dbeta = be.bn_act_bwd(z, None, gamma, y, mean, invstd, dyc, 1, ctx.act, False, True,
                                         into=(None, gg, betag) if direct else None, partial=partial, beta=ctx.beta)
    return dz, None, dgamma, dbeta, None, None, None, None, None, None


class GroupedBNActFn(torch.autograd.Function):
  """The bias / BatchNorm / activation kernels that follow the same-depth dense layers of E parallel stacks
  (GroupedLinearFn) as ONE launch forward and two backward: layer e is BNFromStatsFn (cfg mode BN_BATCH: the statistics its
  GEMM's epilogue produced) or BNActFn (BN_NONE, BN_FROZEN) - same kernels' bodies, same bits, E times fewer launches.
  apply(E, cfgs, z_0.., stats_0.., bias_0.., gamma_0.., beta_0..) -> y_0 .. y_{E-1}; cfgs[e] = (mode, act, moving_mean,
  moving_var, eps, momentum, grad_bufs) with grad_bufs = (bias.grad, gamma.grad, beta.grad) slices of the flat gradient
  buffer or None."""

  @staticmethod
  def forward(ctx, E, cfgs, *args):
    be = hip()
    zs, stats, biases, gammas, betas = (args[i * E:(i + 1) * E] for i in range(5))
    # pres[e] = (y, save [2, N]): layer e was already applied by its contraction's epilogue (GroupedLinearFn, fzs) - only its
    # backward is this Function's
    pres = args[5 * E:6 * E] if len(args) >= 6 * E else (None,) * E
    layers, todo = [], []
    for e in range(E):
      mode, act, mm, mv, eps, momentum, _ = cfgs[e]
      if pres[e] is not None:
        continue
      todo.append(e)
      layers.append(dict(x=zs[e], bias=biases[e], gamma=gammas[e], beta=betas[e], moving_mean=mm, moving_var=mv,
                         col_stats=stats[e], use_bn=mode, act=act, eps=eps, momentum=momentum))
    done = be.bn_fwd_multi(layers) if layers else []
    outs = [None] * E
    for e, o in zip(todo, done):
      outs[e] = o
    for e in range(E):
      if pres[e] is not None:
        y, save = pres[e]
        outs[e] = (y.detach(), save[0], save[1])  # (a new tensor object over the same memory: this Function's output)
    fused = getattr(be, 'fused_bn_bwd', False)
    ctx.owns, saved = [], []
    for e in range(E):
      y, mean, invstd = outs[e]
      mode, act = cfgs[e][0], cfgs[e][1]
      gb = cfgs[e][6]
      own = None
      if fused and mode == BN_BATCH:
        own = BnSource(zs[e], None, y, mean, invstd, act, gammas[e], None if gb is None else (gb[1], gb[2]), beta=betas[e],
                       fused=True)
      elif fused and mode == BN_FROZEN and getattr(be, 'frozen_dz_epilogue', False) and gammas[e] is not None:
        # (z is the bare contraction: the bias enters through zbias)
        own = BnSource(zs[e], None if biases[e] is None else biases[e].detach(), y, mean, invstd, act, gammas[e].detach(), None,
                       beta=betas[e], fused=True)
        own.frozen = True
      ctx.owns.append(own)
      saved += [zs[e], biases[e], gammas[e], betas[e], y, mean, invstd]
    ctx.save_for_backward(*saved)
    ctx.E, ctx.cfgs = E, cfgs
    ctx.n_extra = len(args) - 5 * E
    _bn_tls.last = ctx.owns if any(o is not None for o in ctx.owns) else None  # (the caller tags the outputs)
    return tuple(o[0] for o in outs)

  @staticmethod
  def backward(ctx, *dys):
    be = hip()
    E = ctx.E
    saved = ctx.saved_tensors
    layers = []
    for e in range(E):
      z, bias, gamma, beta, y, mean, invstd = saved[7 * e:7 * e + 7]
      mode, act, gb = ctx.cfgs[e][0], ctx.cfgs[e][1], ctx.cfgs[e][6]
      dy = dys[e] if (dys[e].dim() == 2 and dys[e].stride(1) == 1) else dys[e].contiguous()
      own, partial, dx_done = ctx.owns[e], None, False
      if own is not None:
        # the consumer's input-gradient launch already reduced the column sums, provided dy is exactly its output
        if own.partial is not None and dy.data_ptr() == own.dx_ptr and dy.stride(0) == dy.shape[1]:
          partial = own.partial
          dx_done = own.dz_done  # (... and, on frozen statistics, turned dy into dz: only the parameter gradients are left)
        else:
          assert not own.dz_done, 'a contraction wrote dz for a frozen BatchNorm layer whose backward received another tensor'
        own.partial, own.dz_done = None, False
      into = None
      if gb is not None:
        bg, gg, betag = gb
        if (bias is None or bg is not None) and (gamma is None or (gg is not None and betag is not None)):
          into = (bg if bias is not None else None, gg, betag)
      layers.append(dict(x=z, bias=bias, gamma=gamma, beta=beta, y=y, mean=mean, invstd=invstd, dy=dy, use_bn=mode, act=act,
                         partial=partial, into=into, dx_done=dx_done))
    outs = be.bn_bwd_multi(layers)
    dzs = tuple(o[0] for o in outs)
    none = (None,) * E
    return (None, None) + dzs + none + tuple(o[1] for o in outs) + tuple(o[2] for o in outs) + tuple(o[3] for o in outs) + \
        (None,) * ctx.n_extra


class FMFn(torch.autograd.Function):
  """reference layers/fm.py:20-26 over a [B, F*D] block of the input-layer output."""

  @staticmethod
  def forward(ctx, x, F, D, sink=None, col0=0):
    fm, S = hip().fm_fwd(x, F, D)
    ctx.save_for_backward(x, S)
    ctx.F, ctx.D = F, D
    ctx.sink, ctx.col0 = sink, col0
    return fm

  @staticmethod
  def backward(ctx, g):
    x, S = ctx.saved_tensors
    if ctx.sink is not None:
      # x is (a column block of) an embedding group output: its gradient g * (S - x) is added when the group's gradient
      # buffer is finished (er_group_grad_finish: one launch for all groups and terms)
      ctx.sink.defer(('fm', g if g.stride(-1) == 1 else g.contiguous(), S, ctx.col0, ctx.F * ctx.D, ctx.D))
      return None, None, None, None, None
    dx = hip().fm_bwd(x, S, g.contiguous(), ctx.F, ctx.D)
    if x.shape[1] != ctx.F * ctx.D:
      full = torch.zeros_like(x)
      full[:, :ctx.F * ctx.D] = dx
      dx = full
    return dx, None, None, None, None


class WideFmConcatFn(torch.autograd.Function):
  """DeepFM's [reduce_sum(wide) | FM(fields) | deep] (reference model/deepfm.py:60-83) as one launch; the wide and FM
  blocks live in embedding group outputs, so their gradients are the deferred terms RowSumFn / FMFn would register
  (finished with the group's gradient buffer), and `deep` gets its column block of the incoming gradient as a view."""

  @staticmethod
  def forward(ctx, wide, fm_x, deep, F, D, wide_sink, fm_sink, col0):
    be = hip()
    src = bn_source_of(deep)
    res = None
    if src is not None and src.pending is not None:
      # the deep tower's last BatchNorm finalize + apply rides in this launch (er_bn_apply_wide_fm)
      res = be.bn_apply_wide_fm(src.pending, wide, fm_x, F, D)
      if res is None:
        be.bn_apply_pending(src.pending)
      src.pending = None
    out, S = res if res is not None else be.wide_fm_concat(wide, fm_x, F, D, deep if deep.stride(-1) == 1 else deep.contiguous())
    ctx.save_for_backward(S)
    ctx.F, ctx.D, ctx.n_w = F, D, wide.shape[1]
    ctx.wide_sink, ctx.fm_sink, ctx.col0 = wide_sink, fm_sink, col0
    return out

  @staticmethod
  def backward(ctx, g):
    S, = ctx.saved_tensors
    D = ctx.D
    g = g if g.stride(-1) == 1 else g.contiguous()
    ctx.wide_sink.defer(('rowsum', g[:, 0:1], 0, ctx.n_w))
    ctx.fm_sink.defer(('fm', g[:, 1:1 + D], S, ctx.col0, ctx.F * D, D))
    return None, None, g[:, 1 + D:], None, None, None, None, None


class ConcatFn(torch.autograd.Function):
  """tf.concat(parts, axis=1) (model/deepfm.py:75-83 and the towers' joins): ONE library launch forward; the backward
  hands every producer the column block of the incoming gradient as a VIEW - the fused backward kernels read strided
  gradients in place (no copies)."""

  @staticmethod
  def forward(ctx, *parts):
    ctx.widths = [int(t.shape[1]) for t in parts]
    be = hip()
    st = _bf16_step_state(be)
    ps = [t if t.stride(-1) == 1 else t.contiguous() for t in parts]
    return be.concat_cols(ps, bf16_state=st) if st is not None else be.concat_cols(ps)

  @staticmethod
  def backward(ctx, g):
    out, c = [], 0
    for w in ctx.widths:
      out.append(g[:, c:c + w])
      c += w
    return tuple(out)


def _bf16_step_state(be):
  """The Bf16Shadows of the model being run when its dense part is bf16 with producer-written operands, else None."""
  if not (getattr(be, 'bf16_nt', False) and getattr(be, 'bf16_epilogues', False)):
    return None
  from easyrec_amd.core import context
  stack = context._stack()
  ctx = stack[-1] if stack else None
  if ctx is None or getattr(ctx, 'dense_dtype', 'f32') != 'bf16':
    return None
  return getattr(ctx, 'bf16_state', None)


def concat_cols(parts):
  """Differentiable concat along dim 1 through the library (2-D fp32 tensors)."""
  parts = list(parts)
  if len(parts) == 1:
    return parts[0]
  if any(t.requires_grad for t in parts) and torch.is_grad_enabled():
    out = ConcatFn.apply(*parts)
    # a part that is the output of a fused dense + BatchNorm layer (DCN-v2's deep tower beside the cross stack): the
    # consumer's input-gradient contraction emits that layer's BatchNorm-backward sums from its column block
    c = 0
    for t in parts:
      src = bn_source_of(t)
      if src is not None and src.fused:
        tag_bn_cols(out, t, c)
        break
      c += int(t.shape[1])
    return out
  return hip().concat_cols([t if t.stride(-1) == 1 else t.contiguous() for t in parts])


class DotInteractionFn(torch.autograd.Function):
  """DLRM's pairwise feature interaction (reference model/dlrm.py:44-57) over a contiguous [B, F*D] block."""

  @staticmethod
  def forward(ctx, x, F, D, self_interaction):
    x = x if (x.stride(-1) == 1 and x.dim() == 2) else x.contiguous()
    out = hip().dot_interaction_fwd(x, F, D, self_interaction)
    ctx.save_for_backward(x)
    ctx.F, ctx.D, ctx.self_interaction = F, D, self_interaction
    return out

  @staticmethod
  def backward(ctx, g):
    x, = ctx.saved_tensors
    dx = hip().dot_interaction_bwd(x, g.contiguous(), ctx.F, ctx.D, ctx.self_interaction)
    return dx, None, None, None


class RowSumFn(torch.autograd.Function):
  """reference model/deepfm.py:62-63 (reduce_sum(wide, axis=1, keepdims=True))."""

  @staticmethod
  def forward(ctx, x, sink=None):
    ctx.n = x.shape[1]
    ctx.sink = sink
    return hip().rowsum_fwd(x, x.shape[1])

  @staticmethod
  def backward(ctx, g):
    if ctx.sink is not None:
      ctx.sink.defer(('rowsum', g if g.stride(-1) == 1 else g.contiguous(), 0, ctx.n))
      return None, None
    return hip().rowsum_bwd(g.contiguous(), ctx.n), None


class BNActFn(torch.autograd.Function):
  """bias + BatchNorm(train) + activation: reference layers/dnn.py:57-79.  `grad_bufs` = (bias.grad,
  gamma.grad, beta.grad) slices of the flat gradient buffer: the backward kernel accumulates into them
  directly (no autograd add kernels)."""

  @staticmethod
  def forward(ctx, x, bias, gamma, beta, moving_mean, moving_var, use_bn, eps, momentum, act, training,
              grad_bufs=None):
    mode = BN_NONE
    if use_bn:
      # training=False: the moving statistics normalise and stay as they are - evaluation, and the experts of the
      # reference's MMoE / DBMTL models in TRAINING too (model/mmoe.py:37-47 builds layers/mmoe.py MMOE without
      # is_training); gamma, beta, the bias and the input still receive gradients (er_bn_act_bwd, ER_BN_FROZEN)
      mode = BN_BATCH if training else BN_FROZEN
      assert training or (moving_mean is not None and moving_var is not None)
    y, mean, invstd = hip().bn_act_fwd(x, bias, gamma, beta, mode, eps, momentum, moving_mean, moving_var, act)
    ctx.save_for_backward(x, bias, gamma, y, mean, invstd)
    ctx.cfg = (mode, act)
    ctx.grad_bufs = grad_bufs
    ctx.beta = None if beta is None else beta.detach()  # (read by the backward's mask recomputation only)
    return y

  @staticmethod
  def backward(ctx, dy):
    x, bias, gamma, y, mean, invstd = ctx.saved_tensors
    use_bn, act = ctx.cfg
    into = None
    if ctx.grad_bufs is not None:
      bg, gg, betag = ctx.grad_bufs
      ok = (bias is None or bg is not None) and (gamma is None or (gg is not None and betag is not None))
      if ok:
        into = (bg, gg, betag)
    dx, dbias, dgamma, dbeta = hip().bn_act_bwd(x, bias, gamma, y, mean, invstd, dy.contiguous(), use_bn, act,
                                                bias is not None, gamma is not None, into=into, beta=ctx.beta)
    return dx, dbias, dgamma, dbeta, None, None, None, None, None, None, None, None


class DiceFn(torch.autograd.Function):
  """reference layers/keras/activation.py:47-70 / utils/activation.py:14-44."""

  @staticmethod
  def forward(ctx, x, alpha, moving_mean, moving_var, eps, momentum, alpha_grad=None):
    y, mean, invstd = hip().dice_fwd(x, alpha, eps, momentum, moving_mean, moving_var)
    ctx.save_for_backward(x, alpha, mean, invstd)
    ctx.alpha_grad = alpha_grad
    return y

  @staticmethod
  def backward(ctx, dy):
    x, alpha, mean, invstd = ctx.saved_tensors
    dx, dalpha = hip().dice_bwd(x, alpha, mean, invstd, dy.contiguous())
    if ctx.alpha_grad is not None:
      ctx.alpha_grad.add_(dalpha)
      dalpha = None
    return dx, dalpha, None, None, None, None, None


class CrossV1Fn(torch.autograd.Function):
  """reference model/dcn.py:32-45, all layers in one launch.  `grad_bufs` = ([w_l.grad], [b_l.grad]): the
  per-layer slices of the flat gradient buffer (accumulated into directly; no AccumulateGrad nodes)."""

  @staticmethod
  def forward(ctx, x0, w, b, grad_bufs=None):
    out, dots = hip().cross_v1_fwd(x0.contiguous(), w, b)
    ctx.save_for_backward(x0, w, b, dots)
    ctx.grad_bufs = grad_bufs
    return out

  @staticmethod
  def backward(ctx, dout):
    x0, w, b, dots = ctx.saved_tensors
    dx0, dw, db = hip().cross_v1_bwd(x0.contiguous(), w, b, dots, dout.contiguous())
    if ctx.grad_bufs is not None:
      wg, bg = ctx.grad_bufs
      for i in range(len(wg)):
        wg[i].add_(dw[i])
        bg[i].add_(db[i])
      dw = db = None
    return dx0, dw, db, None


class CrossV2EpilogueFn(torch.autograd.Function):
  """reference layers/keras/interaction.py:276-286: x0 * (u + bias + diag*x) + x.  The backward ADDS its gradients of x0
  and x into the buffers their other consumers use (the embedding group's gradient buffer when x0 is a group output, else
  the tensors' grad_slot): a stack of L cross layers sums nothing through autograd."""

  @staticmethod
  def forward(ctx, x0, x, u, bias, diag_scale, bias_grad=None, sink=None):
    x0c, xc = x0.contiguous(), x.contiguous()
    out = hip().cross_v2_fwd(x0c, xc, u.contiguous(), bias, diag_scale)
    ctx.save_for_backward(x0c, xc, u, bias)
    ctx.diag = diag_scale
    ctx.bias_grad = bias_grad
    ctx.same = x0c.data_ptr() == xc.data_ptr()
    ctx.sink = sink if (sink is not None and x0c is x0) else None
    # (a contiguous copy is another tensor: its consumers do not share a slot)
    ctx.slots = grad_slots_of_step() if (x0c is x0 and xc is x) else None
    return out

  @staticmethod
  def backward(ctx, dout):
    be = hip()
    x0, x, u, bias = ctx.saved_tensors
    d = x0.shape[1]
    ret0 = retx = None
    if not hasattr(be, 'cross_v2_bwd_acc') or ctx.slots is None:
      dx0, dx, du = be.cross_v2_bwd(x0, x, u.contiguous(), bias, ctx.diag, dout.contiguous())
      ret0, retx = dx0, dx
    else:
      # destination of d/dx0: the group's gradient buffer (a first deposit must cover it: here it does), else x0's slot
      sink = ctx.sink
      if sink is not None and sink.covers(0, d):
        t0, acc0 = sink.target(0, d)
      else:
        sink = None
        t0, acc0, first0 = grad_slot(ctx.slots, x0)
        ret0 = t0 if first0 else None
      tx, accx = None, False
      if not ctx.same:
        tx, accx, firstx = grad_slot(ctx.slots, x)
        retx = tx if firstx else None
      dg = dout if (dout.dim() == 2 and dout.stride(1) == 1) else dout.contiguous()  # (a column block of tf.concat's gradient: in place)
      du = be.cross_v2_bwd_acc(x0, x, u.contiguous(), bias, ctx.diag, dg, t0, acc0, tx, accx)
      if sink is not None:
        sink.done()
    dbias = None
    if bias is not None:
      if ctx.bias_grad is not None:  # the column sums straight into the bias' slice of the flat gradient buffer
        be.colsum(du, out=ctx.bias_grad, accumulate=True)
      else:
        dbias = be.colsum(du)
    return ret0, retx, du, dbias, None, None, None


class CrossSrc(object):
  """What the input-gradient contraction of the cross layer ABOVE needs in order to run THIS layer's elementwise backward in
  its epilogue (HipBackend.cross_dgrad_fused(prev=...)), and what it leaves behind for this layer's backward."""
  __slots__ = ('x0', 'x', 'u', 'bias', 'diag', 'bias_grad', 'out', 'sink', 'slots', 'wsink', 'done', 'dout_ptr', 'du', 'ret0')

  def __init__(self, x0, x, u, bias, diag, bias_grad, out, sink, slots, wsink):
    self.x0, self.x, self.u, self.bias, self.diag, self.bias_grad, self.out = x0, x, u, bias, diag, bias_grad, out
    self.sink, self.slots, self.wsink = sink, slots, wsink
    self.done, self.dout_ptr, self.du, self.ret0 = False, 0, None, None

  def dx0_target(self):
    """(tensor, accumulate, what to hand autograd for x0 - the slot tensor on its first use - or None, the sink to mark)"""
    d = self.x0.shape[1]
    sink = self.sink
    if sink is not None and sink.covers(0, d):
      t0, acc0 = sink.target(0, d)
      return t0, acc0, None, sink
    t0, acc0, first0 = grad_slot(self.slots, self.x0)
    return t0, acc0, (t0 if first0 else None), None


_cross_tls = threading.local()


def take_last_cross_source():
  src, _cross_tls.last = getattr(_cross_tls, 'last', None), None
  return src


def cross_source_of(x):
  """The CrossSrc of x if x IS the untouched output of a fused cross layer."""
  src = getattr(x, '_er_cross_src', None)
  if src is None or x.dim() != 2 or x.data_ptr() != src.out.data_ptr() or x.shape != src.out.shape or x.stride() != src.out.stride():
    return None
  return src


class CrossLayerFn(torch.autograd.Function):
  """One full-rank DCN-v2 cross layer x_{l+1} = x0 * (x_l . W + b + diag * x_l) + x_l (reference layers/keras/interaction.py:
  249-286) as ONE launch forward - the contraction with the elementwise part in its epilogue - and, in a stack, ONE launch
  per layer backward: the input-gradient contraction du_l . W^T adds dout_l in its epilogue (the whole gradient of x_{l-1})
  and runs the elementwise backward of the layer below on it (du_{l-1}, d/dx0, the bias gradient's per-tile column sums);
  only the top layer of a stack, whose dout comes from outside, needs its own elementwise launch.  Weight gradients join the
  step's grouped launch; the bias gradients are finished by one launch for all layers (HipBackend.queue_colsum).  d/dx0 goes
  into the embedding group's gradient buffer (sink) or x0's gradient slot."""

  @staticmethod
  def forward(ctx, x0, x, w, bias, diag, w_grad, b_grad, sink, bf16, prev):
    be = hip()
    out, u = be.cross_fwd_fused(x0, x, w, bias, diag, bf16)
    ctx.save_for_backward(x0, x, u, w, bias)
    ctx.diag, ctx.bf16, ctx.w_grad = diag, bf16, w_grad
    ctx.same = x0.data_ptr() == x.data_ptr()
    ctx.prev = prev
    ctx.src = CrossSrc(x0, x, u, bias, diag, b_grad, out, sink, grad_slots_of_step(), be.wgrad_sink())
    _cross_tls.last = ctx.src
    return out

  @staticmethod
  def backward(ctx, dout):
    be = hip()
    x0, x, u, w, bias = ctx.saved_tensors
    src, prev = ctx.src, ctx.prev
    dg = dout if (dout.dim() == 2 and dout.stride(1) == 1) else dout.contiguous()
    ret0 = None
    # 1. this layer's elementwise backward - already done by the contraction of the layer above?
    if src.done and dg.data_ptr() == src.dout_ptr:
      du = src.du
    else:
      t0, acc0, r0, sk = src.dx0_target()
      du, partial = be.cross_bwd_top(x0, x, u, bias, ctx.diag, dg, t0, acc0, ctx.bf16, w)
      if sk is not None:
        sk.done()
      ret0 = r0
      if bias is not None:
        be.queue_colsum(src.wsink, partial, src.bias_grad, bias.numel())
    src.done, src.du = False, None
    # 2. the input-gradient contraction; its epilogue completes the gradient of x_{l-1} and runs the layer below
    retx = None
    if ctx.same:  # x_{l-1} is x0: the gradient joins d/dx0
      t0, acc0, r0, sk = src.dx0_target()
      assert acc0, 'the elementwise backward deposits into d/dx0 first'
      res = be.cross_dgrad_fused(du, w, dg, ctx.diag, ctx.bf16, t0, True)
      assert res is not False
      if sk is not None:
        sk.done()
      ret0 = ret0 if ret0 is not None else r0
    else:
      retx = torch.empty_like(x)
      pv = None
      if prev is not None:
        p0, pacc0, pr0, psk = prev.dx0_target()
        pv = dict(x0=prev.x0, u=prev.u, bias=prev.bias, xl=prev.x, dx0=p0, acc0=pacc0)
      res = be.cross_dgrad_fused(du, w, dg, ctx.diag, ctx.bf16, retx, False, prev=pv)
      assert res is not False
      if prev is not None:
        du_prev, partial_prev = res
        if psk is not None:
          psk.done()
        ret0 = ret0 if ret0 is not None else pr0
        if prev.bias is not None:
          be.queue_colsum(prev.wsink, partial_prev, prev.bias_grad, prev.bias.numel())
        prev.done, prev.dout_ptr, prev.du = True, retx.data_ptr(), du_prev
    # 3. the weight gradient x_{l-1}^T . du joins the step's grouped launch
    dw = None
    if ctx.needs_input_grad[2]:
      dw = _wgrad(be, x, du, ctx.w_grad, ctx.bf16, src.wsink)
    return ret0, retx, dw, None, None, None, None, None, None, None


class CINFn(torch.autograd.Function):
  """xDeepFM's compressed interaction network, all layers (reference layers/keras/interaction.py:370-409).
  x0 [B, H0, D]; kernels[k] [H_k+1, H_k, H0], biases[k] [H_k+1]; returns [B, sum_k H_k+1].  The parameter gradients are
  accumulated into kernel_grads / bias_grads (the flat gradient buffer's views)."""

  @staticmethod
  def forward(ctx, x0, n_layers, *params):
    be = hip()
    kernels, biases = params[:n_layers], params[n_layers:2 * n_layers]
    ctx.kernel_grads, ctx.bias_grads = params[2 * n_layers:3 * n_layers], params[3 * n_layers:4 * n_layers]
    x0 = x0.contiguous()
    B, H0, D = x0.shape
    sizes = [int(w.shape[0]) for w in kernels]
    out = torch.empty(B, sum(sizes), dtype=torch.float32, device=x0.device)
    xi, strides, H = x0, (H0 * D, D, 1), H0
    zs, fms = [], []
    col = 0
    for w, b in zip(kernels, biases):
      N = int(w.shape[0])
      assert w.shape == (N, H, H0), 'cin kernel %s for a [%d x %d] interaction' % (tuple(w.shape), H, H0)
      z = torch.empty(B * D, H * H0, dtype=torch.float32, device=x0.device)
      be.cin_outer_fwd(xi, strides, H, x0, z)
      fm = be.gemm(GEMM_NT, z, w.detach().reshape(N, H * H0))  # [B * D, N] = x_{k+1} as [B, D, N]
      be.cin_act_pool_fwd(fm, b.detach(), B, D, out, col)
      zs.append(z)
      fms.append(fm)
      xi, strides, H = fm, (D * N, 1, N), N
      col += N
    ctx.save_for_backward(x0, *kernels, *zs, *fms)
    ctx.n_layers, ctx.sizes = n_layers, sizes
    return out

  @staticmethod
  def backward(ctx, dout):
    be = hip()
    n = ctx.n_layers
    saved = ctx.saved_tensors
    x0, kernels, zs, fms = saved[0], saved[1:1 + n], saved[1 + n:1 + 2 * n], saved[1 + 2 * n:1 + 3 * n]
    B, H0, D = x0.shape
    dout = dout.contiguous()
    dx0 = torch.zeros_like(x0)
    cols = [sum(ctx.sizes[:k]) for k in range(n)]
    dnext = None  # gradient of x_{k+1} from the layer above ([B * D, N])
    for k in reversed(range(n)):
      w, z, fm = kernels[k].detach(), zs[k], fms[k]
      N = ctx.sizes[k]
      H = H0 if k == 0 else ctx.sizes[k - 1]
      dc = torch.empty_like(fm)
      be.cin_act_pool_bwd(fm, dout, cols[k], dnext, B, D, dc)
      if ctx.bias_grads[k] is not None:
        be.colsum(dc, out=ctx.bias_grads[k], accumulate=True)
      be.gemm(GEMM_TN, dc, z, out=ctx.kernel_grads[k].view(N, H * H0), accumulate=True)  # dW = dc^T . z
      dz = be.gemm(GEMM_NN, dc, w.reshape(N, H * H0))
      if k == 0:
        be.cin_outer_bwd(dz, x0, (H0 * D, D, 1), H, x0, dx0, True, dx0)
        dnext = None
      else:
        prev = fms[k - 1]
        dprev = torch.empty_like(prev)
        be.cin_outer_bwd(dz, prev, (D * H, 1, H), H, x0, dprev, False, dx0)
        dnext = dprev
    return (dx0, None) + (None,) * (4 * n)


class DINConcatFn(torch.autograd.Function):
  """reference model/multi_tower_din.py:69-75: [q, h, q-h, q*h]."""

  @staticmethod
  def forward(ctx, q, h):
    ctx.save_for_backward(q, h)
    # (the history is also read by the pooling: both backward kernels write ONE gradient buffer - kernels.grad_slot)
    ctx.slots = grad_slots_of_step() if h.is_contiguous() else None
    return hip().din_concat_fwd(q.contiguous(), h.contiguous())

  @staticmethod
  def backward(ctx, dout):
    q, h = ctx.saved_tensors
    if ctx.slots is None:
      return hip().din_concat_bwd(q.contiguous(), h.contiguous(), dout.contiguous())
    buf, acc, first = grad_slot(ctx.slots, h)
    dq, _ = hip().din_concat_bwd(q.contiguous(), h, dout.contiguous(), dh=buf, acc_h=acc)
    return dq, (buf if first else None)


class DINFirstLayerFn(torch.autograd.Function):
  """dense (+ bias) -> BatchNorm(train) -> activation over DIN's attention input [q, h, q - h, q * h] ([B, L, 4E], reference
  model/multi_tower_din.py:62-80 feeding layers/dnn.py:57-79) WITHOUT building it, forward or backward: the contraction
  generates the block from (q, h) while staging (er_din_gemm_fwd), the weight gradient likewise (er_din_gemm_wgrad), and the
  input-gradient contraction reduces the block's gradient to dq / dh in its epilogue (er_din_gemm_dgrad).  Same variables
  and arithmetic as LinearBNActFn over DINConcatFn's output; the history's gradient lands in its gradient slot."""

  @staticmethod
  def forward(ctx, q, h, w, b, gamma, beta, moving_mean, moving_var, eps, momentum, act, grad_bufs, defer_apply=False):
    be = hip()
    B, L, E = h.shape
    N = w.shape[1]
    chunks = be.gemm_row_tiles(B * L)
    stats = torch.empty(chunks * N * 3, dtype=torch.float32, device=h.device)
    z = be.din_gemm_fwd(q, h, w, b, col_stats=stats)
    fused = getattr(be, 'fused_bn_bwd', False)
    pend = None
    if defer_apply and fused and getattr(be, 'bn_in_staging', False):
      # the next layer's contraction applies this BatchNorm while it stages its A tiles (LinearBNActFn, HipBackend.gemm_bn_a)
      y = torch.empty_like(z)
      mean = torch.empty(N, dtype=torch.float32, device=z.device)
      invstd = torch.empty(N, dtype=torch.float32, device=z.device)
      pend = dict(z=z, stats=stats, chunks=chunks, gamma=gamma.detach(), beta=beta.detach(), eps=eps, momentum=momentum,
                  moving_mean=moving_mean, moving_var=moving_var, act=act, y=y, mean=mean, invstd=invstd)
    else:
      y, mean, invstd = be.bn_apply_from_stats(z, None, stats, chunks, gamma, beta, eps, momentum, moving_mean, moving_var, act)
    ctx.save_for_backward(q, h, w, gamma, beta, z, y, mean, invstd)
    ctx.act, ctx.grad_bufs = act, grad_bufs
    ctx.slots = grad_slots_of_step()
    gb = None if grad_bufs is None else (grad_bufs[1], grad_bufs[2])
    ctx.own = BnSource(z, None, y, mean, invstd, act, gamma, gb, beta=beta, fused=fused) if fused else None
    if pend is not None:
      ctx.own.pending = pend
    _bn_tls.last = ctx.own
    return y

  @staticmethod
  def backward(ctx, dy):
    be = hip()
    q, h, w, gamma, beta, z, y, mean, invstd = ctx.saved_tensors
    assert ctx.own is None or ctx.own.pending is None, 'a deferred BatchNorm apply was never run (kernels.finish_pending_bn)'
    wg, gg, betag = ctx.grad_bufs if ctx.grad_bufs is not None else (None, None, None)
    direct = gg is not None and betag is not None
    dyc = dy if (dy.dim() == 2 and dy.stride(1) == 1) else dy.contiguous()
    own, partial = ctx.own, None
    if own is not None:
      if own.partial is not None and dyc.data_ptr() == own.dx_ptr:
        partial = own.partial
      own.partial = None
    dz, _, dgamma, dbeta = be.bn_act_bwd(z, None, gamma, y, mean, invstd, dyc, 1, ctx.act, False, True,
                                         into=(None, gg, betag) if direct else None, partial=partial, beta=beta)
    dq = dh = dw = None
    if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
      if ctx.slots is not None:
        buf, acc, first = grad_slot(ctx.slots, h)
        dq, _ = be.din_gemm_dgrad(dz, w, q, h, dh=buf, acc_h=acc)
        dh = buf if first else None
      else:
        dq, dh = be.din_gemm_dgrad(dz, w, q, h)
    if ctx.needs_input_grad[2]:
      if wg is not None:
        be.din_gemm_wgrad(q, h, dz, wg, accumulate=True)
      else:
        dw = be.din_gemm_wgrad(q, h, dz, torch.empty_like(w), accumulate=False)
    return dq, dh, dw, None, dgamma, dbeta, None, None, None, None, None, None, None


class DINPoolFn(torch.autograd.Function):
  """reference model/multi_tower_din.py:86-95: mask, softmax over time, scores @ hist."""

  @staticmethod
  def forward(ctx, scores, hist, seq_len, scale):
    out, probs = hip().din_pool_fwd(scores.contiguous(), hist.contiguous(), seq_len, scale)
    ctx.save_for_backward(probs, hist, seq_len)
    ctx.scale = scale
    ctx.slots = grad_slots_of_step() if hist.is_contiguous() else None
    return out

  @staticmethod
  def backward(ctx, dout):
    probs, hist, seq_len = ctx.saved_tensors
    if ctx.slots is None:
      dscores, dhist = hip().din_pool_bwd(probs, hist.contiguous(), seq_len, dout.contiguous(), ctx.scale)
      return dscores, dhist, None, None
    buf, acc, first = grad_slot(ctx.slots, hist)
    dscores, _ = hip().din_pool_bwd(probs, hist, seq_len, dout.contiguous(), ctx.scale, dhist=buf, acc_h=acc)
    return dscores, (buf if first else None), None, None


class ThetaGradTable(object):
  """The gradient buffers er_theta_grad_reduce writes through, in theta's order: host arrays of their addresses and
  lengths, passed in the launch's kernel arguments (nothing to build on the device, so a first call inside a stream
  capture is fine)."""

  def __init__(self, grads):
    self.grads = list(grads)
    self.table = (ctypes.c_void_p * len(grads))(*[g.data_ptr() for g in grads])
    self.lens = (ctypes.c_int32 * len(grads))(*[g.numel() for g in grads])


class BSTBlockFn(torch.autograd.Function):
  """reference model/multi_tower_bst.py:127-151: the sequence [hist rows (sliced / zero-padded to T - 1), key], the
  multi-head self-attention, add & LayerNorm, the feed-forward dense, add & LayerNorm -> [B, T * E] (er_bst_*).
  apply(key [B, E], hist [B, L, E] (the lookup's static buffer: rows t >= len are zero), seq_len, T, H, grads, *params)
  with params in er_bst_param_count's order and grads their gradient buffers: the parameter gradients are ADDED into
  those (zeroed once per step by VarStore.zero_grad; towers that share variables accumulate in launch order)."""

  @staticmethod
  def forward(ctx, key, hist, seq_len, T, H, grads, *params):
    be = hip()
    E = hist.shape[2]
    theta = _pack_theta(be, params, be.bst_param_count(E, H), 'BSTBlockFn')
    key = key.contiguous()
    out = be.bst_fwd(key, hist, seq_len, theta, T, H)
    ctx.save_for_backward(key, hist, seq_len, theta)
    ctx.T, ctx.H = T, H
    ctx.table = ThetaGradTable(grads) if grads is not None else None
    ctx.slots = grad_slots_of_step() if hist.is_contiguous() else None
    return out

  @staticmethod
  def backward(ctx, dout):
    be = hip()
    key, hist, seq_len, theta = ctx.saved_tensors
    nparams = len(ctx.needs_input_grad) - 6
    assert ctx.table is not None, 'BSTBlockFn: backward without the parameters\' gradient buffers'
    if ctx.slots is None:
      dkey, dhist = be.bst_bwd(key, hist.contiguous(), seq_len, theta, dout.contiguous(), ctx.T, ctx.H, ctx.table)
      return (dkey, dhist, None, None, None, None) + (None,) * nparams
    buf, acc, first = grad_slot(ctx.slots, hist)
    dkey, _ = be.bst_bwd(key, hist, seq_len, theta, dout.contiguous(), ctx.T, ctx.H, ctx.table, dhist=buf, acc_h=acc)
    return (dkey, (buf if first else None), None, None, None, None) + (None,) * nparams


class AutoIntProjFn(torch.autograd.Function):
  """The four bias-free projections of one MultiHeadAttention layer (reference layers/multihead_attention.py:71-95,
  :145-151): x [rows, din] . [Wq | Wk | Wv | Wr] -> [rows, 4d], ONE contraction on an operand packed by one launch.
  Backward: dx is one NT contraction against the packed operand; each weight gradient is x^T . its column slice of the
  incoming gradient, ADDED into the variable's gradient buffer (`grads`, zeroed once per step by VarStore.zero_grad)
  through the step's weight-gradient queue, or returned to autograd when no buffers are given."""

  @staticmethod
  def forward(ctx, x, grads, wq, wk, wv, wr):
    be = hip()
    x = x if x.is_contiguous() else x.contiguous()
    w = be.autoint_pack(wq.detach(), wk.detach(), wv.detach(), wr.detach())
    out = be.gemm(GEMM_NN, x, w)
    ctx.save_for_backward(x, w)
    ctx.grads = grads
    ctx.sink = be.wgrad_sink()
    return out

  @staticmethod
  def backward(ctx, dg):
    be = hip()
    x, w = ctx.saved_tensors
    dg = dg if dg.is_contiguous() else dg.contiguous()
    d = w.shape[1] // 4
    dx = be.gemm(GEMM_NT, dg, w) if ctx.needs_input_grad[0] else None
    dws = [None] * 4
    for k in range(4):
      # (given buffers always receive their gradient; the weights themselves may be detached views)
      if ctx.grads is not None or ctx.needs_input_grad[2 + k]:
        dws[k] = _wgrad(be, x, dg[:, k * d:(k + 1) * d], None if ctx.grads is None else ctx.grads[k], False, ctx.sink)
    return (dx, None) + tuple(dws)


class AutoIntAttnFn(torch.autograd.Function):
  """reference layers/multihead_attention.py:50-161 (use_res) between the projections and the next layer:
  apply(qkvr [B * F, 4d], F, H, ds) -> relu(concat_h softmax(Q_h K_h^T / ds ** -0.5) V_h + R) [B * F, d]
  (er_autoint_attn_fwd / _bwd: the backward recomputes the attention from qkvr; only y is kept)."""

  @staticmethod
  def forward(ctx, qkvr, F, H, ds):
    be = hip()
    qkvr = qkvr if qkvr.is_contiguous() else qkvr.contiguous()
    y = be.autoint_attn_fwd(qkvr, F, H, ds)
    ctx.save_for_backward(qkvr, y)
    ctx.shape = (F, H, ds)
    return y

  @staticmethod
  def backward(ctx, dy):
    qkvr, y = ctx.saved_tensors
    F, H, ds = ctx.shape
    return hip().autoint_attn_bwd(qkvr, y, dy.contiguous(), F, H, ds), None, None, None


class MhaProjFn(torch.autograd.Function):
  """The biased projections of one attention_layer that share an input (reference layers/multihead_cross_attention.py
  :150-177): apply(x [rows, din], grads, n, w_0 .. w_{n-1}, b_0 .. b_{n-1}) -> x . [w_0 | ..] + [b_0 | ..] [rows, n d],
  n = 3 (query | key | value of self-attention) or 2 (key | value of cross-attention): ONE contraction, bias in its
  epilogue, on an operand packed by one launch.  Backward: dx is one NT contraction against the packed operand; each
  weight gradient is x^T . its column slice of the incoming gradient and each bias gradient that slice's column sums,
  ADDED into the variables' gradient buffers (`grads`: the 2 n buffers in the parameters' order, zeroed once per step by
  VarStore.zero_grad), or returned to autograd when no buffers are given."""

  @staticmethod
  def forward(ctx, x, grads, n, *params):
    be = hip()
    assert len(params) == 2 * n
    x = x if x.is_contiguous() else x.contiguous()
    w, bias = be.mha_pack([p.detach() for p in params[:n]], [p.detach() for p in params[n:]])
    out = be.gemm(GEMM_NN, x, w, bias=bias)
    ctx.save_for_backward(x, w)
    ctx.grads, ctx.n = grads, n
    ctx.sink = be.wgrad_sink()
    return out

  @staticmethod
  def backward(ctx, dg):
    be = hip()
    x, w = ctx.saved_tensors
    n = ctx.n
    dg = dg if dg.is_contiguous() else dg.contiguous()
    d = w.shape[1] // n
    dx = be.gemm(GEMM_NT, dg, w) if ctx.needs_input_grad[0] else None
    out = [None] * (2 * n)
    for k in range(n):
      part = dg[:, k * d:(k + 1) * d]
      # (given buffers always receive their gradient; the parameters themselves may be detached views)
      if ctx.grads is not None:
        _wgrad(be, x, part, ctx.grads[k], False, ctx.sink)
        be.colsum(part, out=ctx.grads[n + k], accumulate=True)
      else:
        if ctx.needs_input_grad[3 + k]:
          out[k] = _wgrad(be, x, part, None, False, ctx.sink)
        if ctx.needs_input_grad[3 + n + k]:
          out[n + k] = be.colsum(part)
    return (dx, None, None) + tuple(out)


class MhaAttnFn(torch.autograd.Function):
  """reference layers/multihead_cross_attention.py:179-243 between the projections and the output dense:
  apply(q_src, kv_src, to_mask, B, F, T, H, ds) -> concat_h softmax(Q_h K_h^T / sqrt(ds) + adder) V_h [B * F, H ds].
  kv_src None: q_src is the packed [B * F, 3 H ds] buffer Q | K | V of self-attention (F == T); else q_src [B * F, H ds]
  and kv_src [B * T, 2 H ds] = K | V.  to_mask: int32 [B, T] or None.  The backward (er_mha_bwd) recomputes the
  probabilities and writes dQ | dK | dV into ONE buffer per source, so that the projections' backward is contractions."""

  @staticmethod
  def _split(q_src, kv_src, d):
    if kv_src is None:
      return q_src[:, :d], q_src[:, d:2 * d], q_src[:, 2 * d:3 * d]
    return q_src, kv_src[:, :d], kv_src[:, d:2 * d]

  @staticmethod
  def forward(ctx, q_src, kv_src, to_mask, B, F, T, H, ds):
    return MhaAttnFn._forward(ctx, False, q_src, kv_src, to_mask, B, F, T, H, ds)

  @staticmethod
  def backward(ctx, dctx):
    return MhaAttnFn._backward(ctx, False, dctx)

  @staticmethod
  def _forward(ctx, grouped, q_src, kv_src, to_mask, B, F, T, H, ds):
    be = hip()
    d = H * ds
    q_src = q_src if q_src.is_contiguous() else q_src.contiguous()
    if kv_src is not None:
      kv_src = kv_src if kv_src.is_contiguous() else kv_src.contiguous()
    assert q_src.shape == (B * F, d if kv_src is not None else 3 * d) and (kv_src is not None or F == T)
    assert kv_src is None or kv_src.shape == (B * T, 2 * d)
    q, k, v = MhaAttnFn._split(q_src, kv_src, d)
    out = (be.mha_group_fwd if grouped else be.mha_fwd)(q, k, v, to_mask, B, F, T, H, ds)
    ctx.save_for_backward(q_src, kv_src, to_mask)
    ctx.shape = (B, F, T, H, ds)
    return out

  @staticmethod
  def _backward(ctx, grouped, dctx):
    be = hip()
    q_src, kv_src, to_mask = ctx.saved_tensors
    B, F, T, H, ds = ctx.shape
    d = H * ds
    dq_src = torch.empty_like(q_src)
    dkv_src = None if kv_src is None else torch.empty_like(kv_src)
    q, k, v = MhaAttnFn._split(q_src, kv_src, d)
    dq, dk, dv = MhaAttnFn._split(dq_src, dkv_src, d)
    (be.mha_group_bwd if grouped else be.mha_bwd)(q, k, v, to_mask, dctx.contiguous(), B, F, T, H, ds, dq, dk, dv)
    return dq_src, dkv_src, None, None, None, None, None, None


class MhaGroupAttnFn(MhaAttnFn):
  """MhaAttnFn on the grouped-unit launches (er_mha_group_fwd / _bwd): several (example, head) units per workgroup for
  short sequences (HipBackend.mha_group_units(F, T, ds) >= 2), the same result bits."""

  @staticmethod
  def forward(ctx, q_src, kv_src, to_mask, B, F, T, H, ds):
    return MhaAttnFn._forward(ctx, True, q_src, kv_src, to_mask, B, F, T, H, ds)

  @staticmethod
  def backward(ctx, dctx):
    return MhaAttnFn._backward(ctx, True, dctx)


class SegmentMeanFn(torch.autograd.Function):
  """CMBF's merge_text_embedding and image mean (reference layers/cmbf.py:292-326, :364) as one launch each way:
  apply(x [B, S, W], seg_begin int32 [n_seg + 1] on the device, lens int32 [B, n_seg] or None, n_seg) -> [B, n_seg, W],
  per segment the mean of its first len rows (every row without lens)."""

  @staticmethod
  def forward(ctx, x, seg_begin, lens, n_seg):
    x = x if x.is_contiguous() else x.contiguous()
    ctx.save_for_backward(seg_begin, lens)
    ctx.S = x.shape[1]
    return hip().segment_mean_fwd(x, seg_begin, lens, n_seg)

  @staticmethod
  def backward(ctx, dout):
    seg_begin, lens = ctx.saved_tensors
    return hip().segment_mean_bwd(dout.contiguous(), seg_begin, lens, ctx.S), None, None, None


class AddLayerNormFn(torch.autograd.Function):
  """layer_norm(x + res) of the reference's encoder (layers/multihead_cross_attention.py:346, :365, :768;
  compat/layers.py layer_norm): apply(x [rows, W], res, gamma, beta, eps, grads) -> (x + res - mean) * rstd * gamma +
  beta.  res: None, [rows, W] (the residual) or [S, W] with rows % S == 0 (a per-position addend, read at row % S).
  Backward (er_add_ln_bwd): one launch gives the gradient with respect to x + res, handed to both addends (summed over
  the batch for the broadcast one); dgamma and dbeta are ADDED into `grads` = (gamma's, beta's gradient buffer) by the
  shared fixed-order reduce, or returned to autograd when no buffers are given."""

  @staticmethod
  def forward(ctx, x, res, gamma, beta, eps, grads):
    be = hip()
    x = x if x.is_contiguous() else x.contiguous()
    if res is not None:
      res = res if res.is_contiguous() else res.contiguous()
    y, mean, rstd = be.add_ln_fwd(x, None if res is None else res.detach(), gamma.detach(), beta.detach(), eps)
    ctx.save_for_backward(x, res, gamma, beta, mean, rstd)
    ctx.grads = grads
    return y

  @staticmethod
  def backward(ctx, dy):
    x, res, gamma, beta, mean, rstd = ctx.saved_tensors
    table, acc, ret = _theta_grads(ctx, (gamma, beta))
    dz = hip().add_ln_bwd(dy.contiguous(), x, res, gamma, mean, rstd, table, acc)
    dres = None
    if res is not None and ctx.needs_input_grad[1]:
      dres = dz if res.shape[0] == x.shape[0] else dz.view(-1, res.shape[0], res.shape[1]).sum(dim=0)
    return (dz, dres) + ret + (None, None)


def _pack_theta(be, params, count, what):
  """The block's parameters side by side in one vector (one copy launch)."""
  theta = torch.empty(count, dtype=torch.float32, device=params[0].device)
  pairs, o = [], 0
  for prm in params:
    n = prm.numel()
    pairs.append((theta[o:o + n], prm.detach().reshape(-1)))
    o += n
  assert o == count, '%s: %d parameter floats, the kernel expects %d' % (what, o, count)
  be.copy_multi(pairs)
  return theta


def _theta_grads(ctx, params):
  """-> (table, acc, returned): the gradient buffers the reduce launch writes through.  With the variables' buffers
  (`grads`, zeroed once per step by VarStore.zero_grad) the gradients are ADDED there and autograd gets nothing; without,
  fresh tensors are written and returned to autograd."""
  if ctx.grads is not None:
    return ThetaGradTable(ctx.grads), True, (None,) * len(params)
  fresh = [torch.empty_like(p) for p in params]
  return ThetaGradTable(fresh), False, tuple(fresh)


class BiLinearFn(torch.autograd.Function):
  """reference layers/keras/fibinet.py:175-203 up to the concatenation (types `all` and `each`):
  apply(x [B, F * D], F, D, each, plus, grads, kernel_0, bias_0[, kernel_1, bias_1, ..]) -> the pairs' <u_i, x_j>
  [B, F (F - 1) / 2] (plus) or u_i * x_j [B, F (F - 1) / 2 * D], u_i = x_i kernel_i + bias_i (er_bilinear_*: one
  launch each way and a fixed-order reduce of the parameter gradients; the backward recomputes u)."""

  @staticmethod
  def forward(ctx, x, F, D, each, plus, grads, *params):
    be = hip()
    x = x if x.is_contiguous() else x.contiguous()
    theta = _pack_theta(be, params, be.bilinear_param_count(F, D, each), 'BiLinearFn')
    out = be.bilinear_fwd(x, theta, F, D, each, plus)
    ctx.save_for_backward(x, theta, *params)
    ctx.cfg = (F, D, each, plus)
    ctx.grads = grads
    return out

  @staticmethod
  def backward(ctx, dout):
    x, theta = ctx.saved_tensors[:2]
    F, D, each, plus = ctx.cfg
    table, acc, ret = _theta_grads(ctx, ctx.saved_tensors[2:])
    dx = hip().bilinear_bwd(x, theta, dout.contiguous(), F, D, each, plus, table, acc=acc)
    return (dx, None, None, None, None, None) + ret


class SENetFn(torch.autograd.Function):
  """reference layers/keras/fibinet.py:63-93: apply(x [B, F * D], F, D, G, R, skip, ln, grads, W1, b1, W2, b2[, gamma,
  beta]) -> the re-weighted (+ skip connection) (+ layer-normalised) fields [B, F * D] (er_senet_*: one launch each way
  and a fixed-order reduce of the parameter gradients; the backward recomputes the squeeze and the excitation)."""

  @staticmethod
  def forward(ctx, x, F, D, G, R, skip, ln, grads, *params):
    be = hip()
    x = x if x.is_contiguous() else x.contiguous()
    assert len(params) == (6 if ln else 4)
    theta = _pack_theta(be, params, be.senet_param_count(F, D, G, R, ln), 'SENetFn')
    y = be.senet_fwd(x, theta, F, D, G, R, skip, ln)
    ctx.save_for_backward(x, theta, *params)
    ctx.cfg = (F, D, G, R, skip, ln)
    ctx.grads = grads
    return y

  @staticmethod
  def backward(ctx, dy):
    x, theta = ctx.saved_tensors[:2]
    F, D, G, R, skip, ln = ctx.cfg
    table, acc, ret = _theta_grads(ctx, ctx.saved_tensors[2:])
    dx = hip().senet_bwd(x, theta, dy.contiguous(), F, D, G, R, skip, ln, table, acc=acc)
    return (dx, None, None, None, None, None, None, None) + ret


class MaskMulFn(torch.autograd.Function):
  """reference layers/keras/mask_net.py:100 for the n mask blocks that share one input: apply(x [B, W], v_0, .., v_{n-1})
  -> (x * v_0, .., x * v_{n-1}), one launch each way (er_mask_mul_*).  The v_i are read where their Dense layers wrote
  them (column slices of a wider tensor included).  A caller that does not need the gradient with respect to x (x does
  not require one) gets none, and the launch skips it."""

  @staticmethod
  def forward(ctx, x, *vs):
    outs = hip().mask_mul_fwd(x.detach(), [v.detach() for v in vs])
    ctx.save_for_backward(x, *vs)
    return tuple(outs)

  @staticmethod
  def backward(ctx, *douts):
    x, vs = ctx.saved_tensors[0], list(ctx.saved_tensors[1:])
    douts = [d if d is not None else torch.zeros_like(x) for d in douts]
    dvs, dx = hip().mask_mul_bwd(x, vs, douts, want_dx=ctx.needs_input_grad[0])
    return (dx,) + tuple(dvs)


class LnReluFn(torch.autograd.Function):
  """reference layers/keras/mask_net.py:106-107 for n mask blocks of one output width: apply(eps, grads, out, col0,
  h_0, .., h_{n-1}, gamma_0, beta_0, .., gamma_{n-1}, beta_{n-1}) -> relu(LayerNormalization_i(h_i)) side by side.
  out None: a fresh [B, n * O], the parallel form's concatenation.  out a row-major [B, >= col0 + n * O] buffer: written
  IN PLACE at columns [col0, col0 + n * O) and returned whole (blocks of unequal widths fill one concatenation launch by
  launch; the other columns pass their gradient through).  Backward (er_ln_relu_bwd): the ReLU pattern is the saved
  output's (y > 0); dgamma_i and dbeta_i are ADDED into `grads` = (gamma_0's, beta_0's, gamma_1's, .. gradient buffers)
  by the shared fixed-order reduce, or returned to autograd when no buffers are given."""

  @staticmethod
  def forward(ctx, eps, grads, out, col0, *tensors):
    n = len(tensors) // 3
    assert len(tensors) == 3 * n and n >= 1
    hs, gb = [h.detach() for h in tensors[:n]], [t.detach() for t in tensors[n:]]
    B, O = hs[0].shape
    if out is None:
      y, mean, rstd = hip().ln_relu_fwd(hs, gb[0::2], gb[1::2], eps)
      ret = y
    else:
      assert not out.requires_grad or not out.is_leaf
      y = out.detach()[:, col0:col0 + n * O]
      _, mean, rstd = hip().ln_relu_fwd(hs, gb[0::2], gb[1::2], eps, y=y)
      ctx.mark_dirty(out)
      ret = out
    ctx.save_for_backward(mean, rstd, *tensors)
    # (the saved output is the storage autograd already holds; a later block's in-place write into OTHER columns of the
    # same buffer must not invalidate it, so it is kept as a view and not through save_for_backward - a DETACHED one: the
    # returned tensor itself would own this node and the node it, a cycle that keeps the graph alive until a collection)
    ctx.y = y.detach()
    ctx.grads, ctx.n, ctx.cols = grads, n, (None if out is None else (col0, col0 + n * O))
    return ret

  @staticmethod
  def backward(ctx, dy):
    mean, rstd = ctx.saved_tensors[:2]
    n = ctx.n
    hs, gb = list(ctx.saved_tensors[2:2 + n]), list(ctx.saved_tensors[2 + n:])
    table, acc, ret = _theta_grads(ctx, gb)
    dout = None
    if ctx.cols is not None:
      c0, c1 = ctx.cols
      if dy.stride(-1) != 1:
        dy = dy.contiguous()
      dmine = dy[:, c0:c1]
      if ctx.needs_input_grad[2]:  # (what was in these columns before is overwritten: no gradient reaches it)
        dout = dy.clone()
        dout[:, c0:c1] = 0
    else:
      dmine = dy
    dhs = hip().ln_relu_bwd(dmine, ctx.y, hs, gb[0::2], mean, rstd, table, acc)
    return (None, None, dout, None) + tuple(dhs) + ret


class GateScaleFn(torch.autograd.Function):
  """reference layers/keras/ppnet.py:51-58, :185-187: apply(grads, x [B, W], z [B, W], bias [W] or None) ->
  x * 2 * sigmoid(z + bias), one launch each way (er_gate_scale_*); z is the gate's `weight` Dense before its bias.  The
  backward recomputes the gate.  `grads` = [the bias's gradient buffer]: dbias is ADDED into it by the shared fixed-order
  reduce and autograd gets None for the bias; grads None: dbias is returned.  A caller whose x does not require a
  gradient gets none, and the launch skips it."""

  @staticmethod
  def forward(ctx, grads, x, z, bias):
    out = hip().gate_scale_fwd(x.detach(), z.detach(), None if bias is None else bias.detach())
    ctx.save_for_backward(x, z, *(() if bias is None else (bias,)))
    ctx.grads = grads
    return out

  @staticmethod
  def backward(ctx, dout):
    x, z = ctx.saved_tensors[:2]
    bias = list(ctx.saved_tensors[2:])
    table, acc, ret = _theta_grads(ctx, bias) if bias else (None, False, (None,))
    dx, dz = hip().gate_scale_bwd(dout, x, z, bias[0] if bias else None, table, acc, want_dx=ctx.needs_input_grad[1])
    return (None, dx, dz) + ret


class VDropSeg(object):
  """The column -> parameter map of feature-wise variational dropout, as er_vdrop_* take it: `dims` = the features'
  widths in the concatenation's order -> W = sum(dims) int32 entries, once in a host array (checked by every launch) and
  once on the device (read by the kernel).  Built once per layer."""

  def __init__(self, dims, device):
    seg = np.repeat(np.arange(len(dims), dtype=np.int32), np.asarray(dims, dtype=np.int64))
    self.W = int(seg.size)
    self.host = (ctypes.c_int32 * self.W)(*seg.tolist())
    self.dev = torch.from_numpy(seg).to(device)


class VDropFn(torch.autograd.Function):
  """reference layers/variational_dropout_layer.py:71-130: apply(grads, x [B, W], logit_p [P], u [B, P] or None
  (evaluation), seg (a VDropSeg, or None for the identity: P == W), lam = regularization_lambda / B) -> (x * m, penalty
  [1]), one launch each way (er_vdrop_*).  The backward recomputes m from (logit_p, u).  `grads` = [logit_p's gradient
  buffer]: dlogit_p - the batch sums and the penalty's own gradient - is ADDED into it by the shared fixed-order reduce
  and autograd gets None for logit_p; grads None: dlogit_p is returned.  A caller whose x does not require a gradient
  gets none, and the launch skips it."""

  @staticmethod
  def forward(ctx, grads, x, logit_p, u, seg, lam):
    out, penalty = hip().vdrop_fwd(x.detach(), logit_p.detach(), u, seg, lam)
    ctx.save_for_backward(x, logit_p, *(() if u is None else (u,)))
    ctx.grads, ctx.seg, ctx.lam = grads, seg, lam
    return out, penalty

  @staticmethod
  def backward(ctx, dout, dpenalty):
    x, logit_p = ctx.saved_tensors[:2]
    u = ctx.saved_tensors[2] if len(ctx.saved_tensors) > 2 else None
    table, acc, ret = _theta_grads(ctx, [logit_p])
    dx = hip().vdrop_bwd(dout, dpenalty.reshape(1).contiguous(), x, logit_p.detach(), u, ctx.seg, ctx.lam, table, acc,
                         want_dx=ctx.needs_input_grad[1])
    return (None, dx) + ret + (None, None, None)


def _seq_column(x):
  """x [B, L_buf, D] as the K8h kernels read it: in place when it is a column view of the engine's sequence output."""
  ok = x.stride(2) == 1 and x.stride(1) >= x.shape[2] and x.stride(0) == x.shape[1] * x.stride(1)
  return x if ok else x.contiguous()


class TextCnnFn(torch.autograd.Function):
  """reference layers/keras/blocks.py:243-257 up to the concatenation: apply(x [B, L_buf, D], P, sizes, filters, relu,
  grads, kernel_0, bias_0[, kernel_1, bias_1, ..]) -> [B, sum filters], the maxima over the window positions of
  act(Conv1D_i) of the sequence padded / truncated to P (er_text_cnn_*: one launch each way and a fixed-order reduce of
  the parameter gradients; the backward recomputes the convolutions).  kernel_i [k_i, D, F_i]."""

  @staticmethod
  def forward(ctx, x, P, sizes, filters, relu, grads, *params):
    be = hip()
    x = _seq_column(x)
    assert len(params) == 2 * len(sizes)
    theta = _pack_theta(be, params, be.text_cnn_param_count(x.shape[2], sizes, filters), 'TextCnnFn')
    y = be.text_cnn_fwd(x, theta, P, sizes, filters, relu)
    ctx.save_for_backward(x, theta, *params)
    ctx.cfg = (P, tuple(sizes), tuple(filters), relu)
    ctx.grads = grads
    return y

  @staticmethod
  def backward(ctx, dy):
    x, theta = ctx.saved_tensors[:2]
    P, sizes, filters, relu = ctx.cfg
    table, acc, ret = _theta_grads(ctx, ctx.saved_tensors[2:])
    dx = hip().text_cnn_bwd(x, theta, dy.contiguous(), P, sizes, filters, relu, table, acc=acc)
    return (dx, None, None, None, None, None) + ret


class SeqAttnPoolFn(torch.autograd.Function):
  """reference layers/input_layer.py:323-338: apply(x [B, L_buf, D], seq_len int32 [B], grads, w [D, 1]) -> [B, D], the
  sum over time weighted by softmax(<x_t, w> where t < len, -2^32 + 1 elsewhere) (er_seq_attn_pool_*)."""

  @staticmethod
  def forward(ctx, x, seq_len, grads, w):
    x = _seq_column(x)
    y = hip().seq_attn_pool_fwd(x, seq_len, w.detach().reshape(-1))
    ctx.save_for_backward(x, seq_len, w)
    ctx.grads = grads
    return y

  @staticmethod
  def backward(ctx, dy):
    x, seq_len, w = ctx.saved_tensors
    table, acc, ret = _theta_grads(ctx, (w,))
    dx = hip().seq_attn_pool_bwd(x, seq_len, w.detach().reshape(-1), dy.contiguous(), table, acc=acc)
    return (dx, None, None) + ret


class MatchNormalizeFn(torch.autograd.Function):
  """reference model/match_model.py:141-143, tf.nn.l2_normalize(fea, axis=-1): apply(x [R, D]) -> x / max(|x|, 1e-6)
  per row (er_match_normalize_*: the forward keeps the rows' inverse norms)."""

  @staticmethod
  def forward(ctx, x):
    x = x if x.is_contiguous() else x.contiguous()
    y, inv = hip().match_normalize_fwd(x)
    ctx.save_for_backward(x, inv)
    return y

  @staticmethod
  def backward(ctx, dy):
    x, inv = ctx.saved_tensors
    return hip().match_normalize_bwd(x, inv, dy.contiguous())


class MatchSoftmaxLossFn(torch.autograd.Function):
  """reference model/match_model.py:50-69, :213-234 and model/dssm.py:71-96 from the tower outputs to the two losses:
  apply(U [B, D], I [M, D], inv_temperature, item_ids [M] int64 or None, ignore_in_batch, weight [B] or None, grads,
  sim_w, sim_b) -> (cross_entropy_loss, reg_pos_loss, stats) (er_match_softmax_*: the [B, M] logits are never stored;
  the backward recomputes them from the saved row maxima and sums).  sim_w / sim_b: one-float tensors, or both None for
  no scale; with `grads` (their gradient buffers) their gradients are ADDED there and autograd gets nothing.  stats
  [4, B]: the rows' maximum, sum, diagonal logit and hit probability (not differentiable)."""

  @staticmethod
  def forward(ctx, U, I, inv_temperature, item_ids, ignore_in_batch, weight, grads, sim_w, sim_b):
    be = hip()
    U = U if U.is_contiguous() else U.contiguous()
    I = I if I.is_contiguous() else I.contiguous()
    assert (sim_w is None) == (sim_b is None)
    weight = None if weight is None else weight.contiguous()
    sw = None if sim_w is None else sim_w.detach()
    sb = None if sim_b is None else sim_b.detach()
    losses, stats = be.match_softmax_fwd(U, I, inv_temperature, sw, sb, item_ids, ignore_in_batch, weight)
    ctx.save_for_backward(U, I, item_ids, weight, sw, sb, stats, losses)
    ctx.cfg = (inv_temperature, ignore_in_batch)
    ctx.grads = grads
    ctx.mark_non_differentiable(stats)
    return losses[0], losses[1], stats

  @staticmethod
  def backward(ctx, g_ce, g_reg, _):
    U, I, item_ids, weight, sw, sb, stats, losses = ctx.saved_tensors
    inv_temperature, ignore_in_batch = ctx.cfg
    table, acc, ret = None, True, (None, None)
    if sw is not None:
      table, acc, ret = _theta_grads(ctx, (sw, sb))
    dU, dI = hip().match_softmax_bwd(U, I, inv_temperature, sw, sb, item_ids, ignore_in_batch, weight, stats, losses,
                                     g_ce.reshape(1).contiguous(), g_reg.reshape(1).contiguous(), table, acc)
    return (dU, dI, None, None, None, None, None) + ret


class CapsuleRoutingFn(torch.autograd.Function):
  """reference layers/capsule_layer.py:60-176: apply(hist [B, L, D], seq_len [B] int32, logits0 ([B, S, K] or [S, K]),
  cfg = (S, K, num_iters, routing_logits_scale, squash_pow, scale_ratio, const_caps_num), grads, Smat [D, E]) ->
  (high_capsules [B, K, E], num_caps [B] int32) (er_capsule_*: one launch each way and a fixed-order reduce of capsule/S's
  gradient).  Only the last iteration's routing weights W [B, S, K] are kept: every earlier iteration sits behind
  stop_gradient, and the backward recomputes H = hist Smat and the pre-squash capsules from W.  With `grads` ([Smat's
  gradient buffer]) the gradient is ADDED there and autograd gets nothing."""

  @staticmethod
  def forward(ctx, hist, seq_len, logits0, cfg, grads, Smat):
    S, K, num_iters, scale, squash_pow, scale_ratio, const_caps = cfg
    hist = hist if hist.is_contiguous() else hist.contiguous()
    sm = Smat.detach()
    sm = sm if sm.is_contiguous() else sm.contiguous()
    high, ncaps, W = hip().capsule_fwd(hist, seq_len, sm, logits0, S, K, num_iters, scale, squash_pow, scale_ratio,
                                       const_caps)
    ctx.save_for_backward(hist, seq_len, sm, W)
    ctx.cfg = (squash_pow, scale_ratio, const_caps)
    ctx.grads = grads
    ctx.mark_non_differentiable(ncaps)
    return high, ncaps

  @staticmethod
  def backward(ctx, d_high, _):
    hist, seq_len, sm, W = ctx.saved_tensors
    squash_pow, scale_ratio, const_caps = ctx.cfg
    table, acc, ret = _theta_grads(ctx, (sm,))
    dhist = hip().capsule_bwd(hist, seq_len, sm, W, d_high.contiguous(), squash_pow, scale_ratio, const_caps, table,
                              acc=acc)
    return (dhist, None, None, None, None) + ret


class MindAttentionFn(torch.autograd.Function):
  """reference model/mind.py:168-200, the label-aware attention: apply(interests [B, K, E], pos_item [B, E], num_caps [B]
  int32, simi_pow) -> (user_emb [B, E], user_interests [B, K, E]: the interests with the rows h >= num_caps zero)
  (er_mind_attention_*; the forward keeps the [B, K] weights).  With simi_pow >= 100 the weights are the one-hot of the
  argmax and carry no gradient."""

  @staticmethod
  def forward(ctx, interests, pos_item, num_caps, simi_pow):
    interests = interests if interests.is_contiguous() else interests.contiguous()
    pos_item = pos_item if pos_item.is_contiguous() else pos_item.contiguous()
    emb, ui, w = hip().mind_attention_fwd(interests, pos_item, num_caps, simi_pow)
    ctx.save_for_backward(interests, pos_item, num_caps, w)
    ctx.simi_pow = simi_pow
    ctx.set_materialize_grads(False)
    return emb, ui

  @staticmethod
  def backward(ctx, d_emb, d_ui):
    interests, pos_item, num_caps, w = ctx.saved_tensors
    if d_emb is None:
      d_emb = torch.zeros_like(pos_item)
    di, dp = hip().mind_attention_bwd(interests, pos_item, num_caps, w, d_emb.contiguous(),
                                      None if d_ui is None else d_ui.contiguous(), ctx.simi_pow)
    return di, dp, None, None


class MMoEMixManyFn(torch.autograd.Function):
  """MMoEMixFn over E + T separate tensors: apply(E, T, expert_0 .. expert_{E-1} [B, H], gate_logits_0 .. [B, E]) -> T
  mixtures [B, H].  The inputs are gathered into the kernels' [E, B, H] / [T, B, E] operands by ONE copy launch
  (er_copy_multi) and so are the T output gradients on the way back; the input gradients are views of the backward
  kernels' outputs (torch.stack / select through autograd was ~9 launches of zero-fill and slice copies per step)."""

  @staticmethod
  def forward(ctx, E, T, *args):
    be = hip()
    outs, gate_logits = args[:E], args[E:E + T]
    B, H = outs[0].shape
    dev = outs[0].device
    experts = torch.empty(E, B, H, dtype=torch.float32, device=dev)
    logits = torch.empty(T, B, E, dtype=torch.float32, device=dev)
    be.copy_multi([(experts[e], outs[e] if outs[e].is_contiguous() else outs[e].contiguous()) for e in range(E)] +
                  [(logits[t], gate_logits[t] if gate_logits[t].is_contiguous() else gate_logits[t].contiguous())
                   for t in range(T)])
    out, gates = be.mmoe_mix_fwd(experts, logits)
    ctx.save_for_backward(experts, gates)
    ctx.E, ctx.T = E, T
    return tuple(out[t] for t in range(T))

  @staticmethod
  def backward(ctx, *douts):
    be = hip()
    experts, gates = ctx.saved_tensors
    E, T = ctx.E, ctx.T
    dout = torch.empty(T, experts.shape[1], experts.shape[2], dtype=torch.float32, device=experts.device)
    be.copy_multi([(dout[t], douts[t] if douts[t].is_contiguous() else douts[t].contiguous()) for t in range(T)])
    dexperts, dlogits = be.mmoe_mix_bwd(experts, gates, dout)
    return (None, None) + tuple(dexperts[e] for e in range(E)) + tuple(dlogits[t] for t in range(T))


class MMoEMixFn(torch.autograd.Function):
  """reference layers/mmoe.py:73-82: softmax gates, weighted sum of experts, all tasks at once."""

  @staticmethod
  def forward(ctx, experts, gate_logits):
    out, gates = hip().mmoe_mix_fwd(experts.contiguous(), gate_logits.contiguous())
    ctx.save_for_backward(experts, gates)
    return out

  @staticmethod
  def backward(ctx, dout):
    experts, gates = ctx.saved_tensors
    return hip().mmoe_mix_bwd(experts.contiguous(), gates, dout.contiguous())
