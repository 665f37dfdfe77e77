"""Cases, fp64 references and derived error bounds for the dense-layer family: bias + BatchNorm (batch statistics or the
frozen moving ones) + activation, Dice, the statistics the contractions' epilogues emit and the backward column sums.
No backend is imported here: tests/test_dense_restatement.py (CPU) and tests/test_dense_gpu.py hand one to the run_*
functions.  ratio / ratios / check / U / f32 are tests/_interaction_cases.py's, and so are the conventions: U = 2**-24,
a chain of n operations counted once (n U), an elementwise operation 2 U, M the formula with every term replaced by its
absolute value, a bound of exactly 0 demands equality.

Formulas (layers/dnn.py of the reference: BiasAdd, tf.nn.moments, batch_normalization, Relu; activation.py: Dice),
evaluated in float64 from the float32 inputs, every gradient torch.autograd of them:
  z = x + b;  mu = sum(z) / B;  var = sum((z - mu)^2) / B (biased);  r = 1 / sqrt(var + eps);
  y = act((z - mu) r gamma + beta);  moving <- moving - (moving - value) (1 - momentum).
  Frozen (use_bn == 2): mu, var are the moving statistics, constants; they must come back bit-identical.
  Dice: p = sigmoid((x - mu) r), y = alpha (1 - p) x + p x, gradients through mu and r.
  The ReLU mask is an INPUT of the backward ABI (it reads y): the reference backward is autograd of pre * mask with the
  mask taken from the y tensor handed to the backward, so no element is excluded and none is compared across a flipped
  mask; the forward's own sign pattern is checked by sign_mismatches (it may differ from fp64's only where
  |pre| <= bound(y)).
  The backward is chained from the forward under test (it reads that forward's save_mean / save_invstd / y), as the
  product runs it; its bound therefore carries the forward's d_mu and d_r.

Bounds, per column (za = |x| + |b|, dev = |z - mu|, mean() over the B rows):
  d_mu  = (B + 4) U mean(za)                 B terms; the bias addition and the division: c = 4.
  d_var = (B + 8) U var                      B terms; subtraction, square, division, one spare: c = 8
        + 4 U mean((za + |mu|) dev)          the cancellation in z - mu: z carries U za from the bias addition and mu
                                             is a rounded float (U |mu|); d((z - mu)^2) = 2 dev d(z - mu); 2 U per term
        + 2 d_mu mean(dev) + d_mu^2          the effect of d_mu.  A two-pass evaluation sees only d_mu^2; a merge of
                                             partial (count, mean, M2) records (Chan) sees delta = mean_a - mean_b with
                                             the partial means' own errors, 2 |delta| d(delta) n_a n_b / n <= 2 d_mu
                                             mean(dev) B at worst (two halves): any merge order stays inside.
    There is NO U mean(z^2) term: E[z^2] - mu^2 in float32 rounds E[z^2] and mu^2 to U mu^2 each and exceeds the bound
    by about |mu| / (B sigma) times the rounding it happens to meet - hundreds at mu / sigma = 1000, B = 33.
  d_r / r = d_var / (2 (var + eps)) + 6 U    the addition of eps, sqrtf, the division: c = 6.
  e_d   = 2 U za [only with a bias] + d_mu + 2 U dev          the error of z - mu
  e_xh  = r e_d + (d_r / r + 2 U) r dev                        ... of xhat = (z - mu) r
  y:  |gamma| e_xh + 2 U |gamma| r dev + 2 U (|gamma| r dev + |beta|);  relu is 1-Lipschitz.  Without BatchNorm 2 U za.
  moving: (1 - momentum) d_value + 6 U (|v| + (1 - momentum)(|v| + |value|))   (momentum is a float32 in the case, and
          1 - momentum is then exact in float32 by Sterbenz); three operations: c = 6.
  Frozen: d_mu = 0, d_var = 0, d_r / r = 6 U; save_mean is a copy (bound 0), the moving statistics bound 0.
  backward, g = dy * mask (exact), xhat on the float32 save_mean / save_invstd (e_xh above):
    sg  = sum g:        d_sg  = B U sum|g|
    sgx = sum g xhat:   d_sgx = sum(|g| e_xh) + (B + 2) U sum(|g| |xhat|)
    dx  = gamma r (g - sg / B - xhat sgx / B):  T1 = sg / B (1 / B and a product: 4 U), T2 = xhat (sgx / B) (4 U inside, 2 U
          outside, e_xh on xhat), two subtractions 4 U on M_in = |g| + sum|g| / B + |xhat| sum|g xhat| / B, then two
          products and r's own error: (d_r / r + 4 U) M_in.
    dgamma = sgx, dbeta = sg.  dbias: with batch statistics the gradient is identically zero (the kernels write 0.0;
          autograd leaves rounding noise): bound = the column sum of dx's bound; an accumulate-into buffer must stay
          untouched (bound 0).  Frozen: dx = gamma r g ((d_r / r + 4 U) |gamma| r |g|), dbias = gamma r sg.
          Without BatchNorm dx = g (bound 0), dbias = sg.
    accumulate-into: one more addition, 2 U (|old| + M).
  bf16 copies (yb, dxb): the fp32 bound plus one bfloat16 rounding (2**-8 relative) of the value: bound (1 + 2**-8) +
    2**-8 |reference|.
  Dice: dp = p (1 - p) (e_xh + EXP_U U) + 4 U p + FLT_MIN (an argument error is a relative error of expf, expf at
    EXP_U, the addition and the division); y: (|alpha| + 1) |x| dp + 8 U M_y (subtraction, two products, the addition),
    M_y = |alpha| (1 + p) |x| + p |x|.  Backward, in M form ((1 - a) -> 1 + |a|):
      direct = dy (alpha + (1 - alpha) p): |dy| (1 + |alpha|) dp + 8 U |dy| (|alpha| + (1 + |alpha|) p)
      q = dy x (1 - alpha) p (1 - p): |dy x| (1 + |alpha|) (dp (1 + p) + p (dp + 2 U (1 + p))) + 10 U M_q
      through the statistics as BatchNorm's dx with g = q, d_g = d_q, gamma = 1; dx = direct + that: 2 U more.
      dalpha = sum dy (1 - p) x: sum |dy x| (dp + 2 U (1 + p)) + (B + 4) U sum |dy| (1 + p) |x|.
  Emitted statistics / backward column sums: the same d_mu, d_var (b absent: z is data) and d_sg, d_sgx (mean and
    invstd are data there: e_xh = r (2 U za [with a bias] + 2 U dev) + 2 U r dev).
"""
import functools
import zlib

import torch

from tests._interaction_cases import EXP_U, F32, F64, FLT_MIN, U, _grads, _t, f32

BN_NONE, BN_BATCH, BN_FROZEN = 0, 1, 2   # = easyrec_amd.kernels / oracle.kernel_ref (asserted by the tests)
ACT_NONE, ACT_RELU = 0, 1
EPS, MOM = f32(1e-3), f32(0.99)
BF16_U = 2.0**-8
DY_PAD = 3   # dy as the columns [2, 2 + N) of a [B, N + 3] matrix


# ------------------------------------------------------------------------------------------------------------------
# the library's host arithmetic, restated so that a case can say which path it reaches (er_dense.hip, er_gemm.hip); the
# tests hold these to er_bn_row_chunks / er_bn_apply_row_tiles / er_gemm_row_tiles of the built library
# ------------------------------------------------------------------------------------------------------------------
K_INLINE_CHUNKS, K_MERGE_SLICES, K_APPLY_ROWS, GEMM_BM = 256, 64, 16, 64


def choose_chunks(B, N):
  col_blocks = -(-N // 64)
  return max(1, min(1024 // col_blocks, -(-B // 32), 1024))


def rows_per_chunk(B, N):
  return -(-B // choose_chunks(B, N))


def apply_tiles_per_block(B):
  return 16 if B > 32768 else (4 if B >= 8192 else 1)


def gemm_row_tiles(M):
  return -(-M // GEMM_BM)


# ------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------
def _gen_of(cid):
  return torch.Generator().manual_seed(zlib.crc32(cid.encode()))


def _data(kind, g, B, N, head):
  """x and bias [N] for a data edge.  head: the rows that sit apart in 'head0'."""
  rn = lambda *s: torch.randn(*s, generator=g, dtype=F32)  # noqa: E731
  bias = 0.5 * rn(N)
  if kind == 'randn':
    x = rn(B, N) * 2 + 0.5
  elif kind == 'mean1000':       # z ~ 1000 + randn
    x = 1000.0 + rn(B, N)
  elif kind == 'bigbias':        # z ~ 300 + 0.1 randn, the 300 through the bias
    x, bias = 0.1 * rn(B, N), 300.0 + rn(N)
  elif kind == 'const':          # column 0 constant, the others ordinary
    x = rn(B, N) * 2 + 0.5
    x[:, 0] = 3.25
  elif kind == 'head0':          # the first `head` rows at mean 0, every other row at 1000 +- 1
    x = 1000.0 + (2 * torch.rand(B, N, generator=g, dtype=F32) - 1)
    x[:head] = rn(min(head, B), N)
    bias = torch.zeros(N)
  elif kind == 'drift':          # a linear drift down the rows, 0 -> 1000
    x = torch.linspace(0, 1000, B, dtype=F32)[:, None] + rn(B, N)
  elif kind == 'mixed':          # 1e-3 and 1e3 scales in one column
    big = torch.rand(B, N, generator=g) < 0.5
    x = rn(B, N) * torch.where(big, torch.tensor(1e3), torch.tensor(1e-3))
  else:
    raise ValueError(kind)
  return x, bias


def bn_tensors(cid, B, N, data='randn', head=64, bias=True, affine=True, dy_wide=False, mode=BN_BATCH):
  """Every tensor a BatchNorm / Dice case reads.  gamma[0] = 0 and gamma[1] < 0 (N >= 3); beta[2] = -50 masks every dy of
  column 2 under ReLU."""
  g = _gen_of(cid)
  x, b = _data(data, g, B, N, head)
  rn = lambda *s: torch.randn(*s, generator=g, dtype=F32)  # noqa: E731
  gamma = torch.rand(N, generator=g, dtype=F32) + 0.5
  beta = 0.3 * rn(N)
  if N >= 3:
    gamma[0], gamma[1], beta[2] = 0.0, -1.5, -50.0
  z = x.double() + (b.double() if bias else 0.0)
  if mode == BN_FROZEN:  # moving statistics near the batch's own, so that the normalised values stay O(1)
    mm = (z.mean(0) + 0.1 * z.std(0, unbiased=False) * rn(N).double()).to(F32)
    mv = (z.var(0, unbiased=False) * (0.8 + 0.4 * torch.rand(N, generator=g)).double() + 0.01).to(F32)
  else:
    mm, mv = 0.2 * rn(N), torch.rand(N, generator=g, dtype=F32) + 0.3
  dyw = rn(B, N + DY_PAD)
  t = dict(x=x, bias=b if bias else None, gamma=gamma if affine else None, beta=beta if affine else None, mm=mm, mv=mv,
           dyw=dyw, dy_wide=dy_wide, alpha=0.25 + 0.5 * rn(N),
           old=dict(dbias=rn(N), dgamma=rn(N), dbeta=rn(N)))
  return t


def dy_of(t, dev='cpu'):
  dyw = t['dyw'].to(dev)
  N = t['x'].shape[1]
  return dyw[:, 2:2 + N] if t['dy_wide'] else dyw[:, 2:2 + N].contiguous()


# ------------------------------------------------------------------------------------------------------------------
# BatchNorm: formula
# ------------------------------------------------------------------------------------------------------------------
def _opt(t, k, dt, grad=True):
  return None if t[k] is None else (_t(t[k], dt).requires_grad_(True) if grad else _t(t[k], dt))


def bn_forward(t, mode, act, dt):
  """The forward in dtype dt -> (outputs, graph): graph holds the differentiable pieces for bn_backward."""
  x, b, gamma, beta = _opt(t, 'x', dt), _opt(t, 'bias', dt), _opt(t, 'gamma', dt), _opt(t, 'beta', dt)
  B = x.shape[0]
  z = x if b is None else x + b
  out = {}
  if mode == BN_NONE:
    pre = z
  else:
    mm, mv = _t(t['mm'], dt), _t(t['mv'], dt)
    if mode == BN_FROZEN:
      mu, var = mm, mv
      out['mm'], out['mv'] = mm, mv
    else:
      mu = z.sum(dim=0) / B
      var = ((z - mu)**2).sum(dim=0) / B
      om = 1.0 - MOM if dt == F64 else torch.tensor(1.0, dtype=dt) - torch.tensor(MOM, dtype=dt)
      out['mm'] = mm - (mm - mu) * om
      out['mv'] = mv - (mv - var) * om
    r = 1.0 / torch.sqrt(var + EPS)
    pre = (z - mu) * r
    if gamma is not None:
      pre = pre * gamma + beta
    out['save_mean'], out['save_invstd'] = mu, r
  out['y'] = torch.relu(pre) if act == ACT_RELU else pre
  graph = dict(x=x, b=b, gamma=gamma, beta=beta, pre=pre)
  return {k: v.detach() for k, v in out.items()}, graph


def bn_backward(t, mode, act, dt, graph, y_given):
  """autograd of pre * mask, the mask from y_given (the tensor the backward under test reads) -> dx, dbias, dgamma, dbeta
  and the accumulate-into forms."""
  pre = graph['pre']
  out = pre * (y_given.detach().to('cpu', dt) > 0).to(dt) if act == ACT_RELU else pre
  wrt = [graph['x']] + [graph[k] for k in ('b', 'gamma', 'beta') if graph[k] is not None]
  gr = list(_grads(out, wrt, _t(dy_of(t), dt)))
  res = dict(dx=gr.pop(0))
  for k, name in (('b', 'dbias'), ('gamma', 'dgamma'), ('beta', 'dbeta')):
    if graph[k] is not None:
      gv = gr.pop(0)
      res[name] = torch.zeros_like(graph[k]) if gv is None else gv
  for name in ('dbias', 'dgamma', 'dbeta'):
    if name in res:
      old = _t(t['old'][name], dt)
      # batch statistics remove the column mean: the bias has NO gradient and its buffer must stay untouched
      res['acc_' + name] = old.clone() if (name == 'dbias' and mode == BN_BATCH) else old + res[name]
  return {k: v.detach() for k, v in res.items()}


def bn_plain(t, mode, act, dt):
  """Forward and the backward chained from it, all in dt (float32: the plain evaluation held to half the bound)."""
  fwd, graph = bn_forward(t, mode, act, dt)
  fwd.update(bn_backward(t, mode, act, dt, graph, fwd['y']))
  return fwd


# ------------------------------------------------------------------------------------------------------------------
# BatchNorm: bounds
# ------------------------------------------------------------------------------------------------------------------
def _stats_bound(za, z, mu, var, B, has_bias, frozen):
  """-> dict(dev, d_mu, d_var, dr_rel, e_xh): the statistics' errors and xhat's, fp64 tensors."""
  dev = (z - mu).abs()
  if frozen:
    d_mu, d_var = torch.zeros_like(mu), torch.zeros_like(var)
  else:
    d_mu = (B + 4) * U * za.mean(dim=0)
    d_var = (B + 8) * U * var + 4 * U * ((za + mu.abs()) * dev).mean(dim=0) + 2 * d_mu * dev.mean(dim=0) + d_mu**2
  dr_rel = 0.5 * d_var / (var + EPS) + 6 * U
  r = 1.0 / torch.sqrt(var + EPS)
  e_d = (2 * U * za if has_bias else 0.0) + d_mu + 2 * U * dev
  e_xh = r * e_d + (dr_rel + 2 * U) * r * dev
  return dict(dev=dev, d_mu=d_mu, d_var=d_var, dr_rel=dr_rel, r=r, e_xh=e_xh)


def _dx_bound(g_abs, d_g, xh_abs, e_xh, r, dr_rel, ga_abs, B):
  """Bound of ga r (g - sum(g) / B - xhat sum(g xhat) / B) -> (dx bound, d_sg, d_sgx, sum|g|, sum|g xhat|)."""
  Asg, Asgx = g_abs.sum(dim=0), (g_abs * xh_abs).sum(dim=0)
  d_sg = d_g.sum(dim=0) + B * U * Asg
  d_sgx = (d_g * xh_abs + g_abs * e_xh).sum(dim=0) + (B + 2) * U * Asgx
  T1, T2 = Asg / B, xh_abs * Asgx / B
  dT1 = d_sg / B + 4 * U * T1
  dT2 = e_xh * Asgx / B + xh_abs * (d_sgx / B + 4 * U * Asgx / B) + 2 * U * T2
  Min = g_abs + T1 + T2
  d_in = d_g + dT1 + dT2 + 4 * U * Min
  return ga_abs * r * (d_in + (dr_rel + 4 * U) * Min), d_sg, d_sgx, Asg, Asgx


def bn_bound(t, mode, act, y_given):
  x = _t(t['x'], F64)
  B = x.shape[0]
  has_bias = t['bias'] is not None
  b = _t(t['bias'], F64) if has_bias else torch.zeros(x.shape[1], dtype=F64)
  z, za = x + b, x.abs() + b.abs()
  ga = _t(t['gamma'], F64).abs() if t['gamma'] is not None else torch.ones(x.shape[1], dtype=F64)
  be = _t(t['beta'], F64).abs() if t['beta'] is not None else torch.zeros(x.shape[1], dtype=F64)
  g_abs = _t(dy_of(t), F64).abs()
  if act == ACT_RELU:
    g_abs = g_abs * (y_given.detach().to('cpu', F64) > 0).to(F64)
  old = {k: _t(v, F64).abs() for k, v in t['old'].items()}
  bd = {}
  if mode == BN_NONE:
    bd['y'] = 2 * U * za if has_bias else torch.zeros_like(z)
    bd['dx'] = torch.zeros_like(z)
    if has_bias:
      Asg = g_abs.sum(dim=0)
      bd['dbias'] = B * U * Asg
      bd['acc_dbias'] = bd['dbias'] + 2 * U * (old['dbias'] + Asg)
    return bd
  frozen = mode == BN_FROZEN
  mm, mv = _t(t['mm'], F64), _t(t['mv'], F64)
  mu, var = (mm, mv) if frozen else (z.mean(dim=0), z.var(dim=0, unbiased=False))
  s = _stats_bound(za, z, mu, var, B, has_bias, frozen)
  r, dev, e_xh = s['r'], s['dev'], s['e_xh']
  bd['save_mean'] = s['d_mu']
  bd['save_invstd'] = r * s['dr_rel']
  if frozen:
    bd['mm'], bd['mv'] = torch.zeros_like(mm), torch.zeros_like(mv)
  else:
    om = 1.0 - MOM
    bd['mm'] = om * s['d_mu'] + 6 * U * (mm.abs() + om * (mm.abs() + mu.abs()))
    bd['mv'] = om * s['d_var'] + 6 * U * (mv.abs() + om * (mv.abs() + var))
  bd['y'] = ga * e_xh + 2 * U * ga * r * dev + 2 * U * (ga * r * dev + be)
  xh_abs = r * dev
  zero = torch.zeros_like(g_abs)
  dxb, d_sg, d_sgx, Asg, Asgx = _dx_bound(g_abs, zero, xh_abs, e_xh, r, s['dr_rel'], ga, B)
  if frozen:
    bd['dx'] = (s['dr_rel'] + 4 * U) * ga * r * g_abs
    if has_bias:
      bd['dbias'] = ga * r * (d_sg + (s['dr_rel'] + 4 * U) * Asg)
      bd['acc_dbias'] = bd['dbias'] + 2 * U * (old['dbias'] + ga * r * Asg)
  else:
    bd['dx'] = dxb
    if has_bias:
      bd['dbias'] = dxb.sum(dim=0)
      bd['acc_dbias'] = torch.zeros_like(Asg)
  if t['gamma'] is not None:
    bd['dgamma'], bd['dbeta'] = d_sgx, d_sg
    bd['acc_dgamma'] = d_sgx + 2 * U * (old['dgamma'] + Asgx)
    bd['acc_dbeta'] = d_sg + 2 * U * (old['dbeta'] + Asg)
  return bd


def bf16_bound(bound, ref):
  """The bound of a bfloat16 copy of a tensor held to `bound`: one more rounding, 2**-8 relative."""
  return bound * (1 + BF16_U) + BF16_U * ref.abs()


def sign_mismatches(y_got, t, mode, act, pre=None):
  """Elements where the forward's sign pattern (y > 0) differs from fp64's although |pre| is above y's bound.
  pre: the fp64 pre-activation when the caller holds it already."""
  if act != ACT_RELU:
    return 0
  if pre is None:
    pre = bn_forward(t, mode, ACT_NONE, F64)[1]['pre']
  pre = pre.detach()
  bound = bn_bound(t, mode, ACT_NONE, pre)['y']
  differs = (y_got.detach().to('cpu', F64) > 0) != (pre > 0)
  return int((differs & (pre.abs() > bound)).sum())


# ------------------------------------------------------------------------------------------------------------------
# emitted statistics and backward column sums, the produced tensors taken as data
# ------------------------------------------------------------------------------------------------------------------
def stats_reference(z):
  """z [B, N] (what the contraction wrote) -> fp64 (mean, biased variance) and their bounds."""
  zd = _t(z, F64).cpu()
  B = zd.shape[0]
  mu, var = zd.mean(dim=0), zd.var(dim=0, unbiased=False)
  s = _stats_bound(zd.abs(), zd, mu, var, B, False, False)
  return dict(mean=mu, var=var), dict(mean=s['d_mu'], var=s['d_var'])


def colsum_reference(dy, z, zbias, y, mean, invstd, act):
  """sum g and sum g xhat in fp64 from the float32 tensors handed to the contraction (mean / invstd None: no BatchNorm,
  the second sum is not defined and not returned) and their bounds."""
  c = lambda v: _t(v, F64).cpu()  # noqa: E731
  g = c(dy)
  B = g.shape[0]
  if act == ACT_RELU:
    g = g * (c(y) > 0).to(F64)
  ref, bd = dict(sg=g.sum(dim=0)), dict(sg=B * U * g.abs().sum(dim=0))
  if mean is not None:
    zz = c(z) + (c(zbias) if zbias is not None else 0.0)
    za = c(z).abs() + (c(zbias).abs() if zbias is not None else 0.0)
    r = c(invstd)
    d = zz - c(mean)
    xh = d * r
    e_xh = r.abs() * ((2 * U * za if zbias is not None else 0.0) + 2 * U * d.abs()) + 2 * U * xh.abs()
    ref['sgx'] = (g * xh).sum(dim=0)
    bd['sgx'] = (g.abs() * e_xh).sum(dim=0) + (B + 2) * U * (g.abs() * xh.abs()).sum(dim=0)
  return ref, bd


# ------------------------------------------------------------------------------------------------------------------
# Dice
# ------------------------------------------------------------------------------------------------------------------
def dice_plain(t, dt):
  x, alpha = _opt(t, 'x', dt), _opt(t, 'alpha', dt)
  B = x.shape[0]
  mu = x.sum(dim=0) / B
  var = ((x - mu)**2).sum(dim=0) / B
  r = 1.0 / torch.sqrt(var + EPS)
  p = torch.sigmoid((x - mu) * r)
  y = alpha * (1.0 - p) * x + p * x
  mm, mv = _t(t['mm'], dt), _t(t['mv'], dt)
  om = 1.0 - MOM if dt == F64 else torch.tensor(1.0, dtype=dt) - torch.tensor(MOM, dtype=dt)
  dx, dalpha = _grads(y, (x, alpha), _t(dy_of(t), dt))
  res = dict(y=y, save_mean=mu, save_invstd=r, mm=mm - (mm - mu) * om, mv=mv - (mv - var) * om, dx=dx, dalpha=dalpha)
  return {k: v.detach() for k, v in res.items()}


def dice_bound(t):
  x, al = _t(t['x'], F64), _t(t['alpha'], F64)
  B = x.shape[0]
  xa, aa, dya = x.abs(), al.abs(), _t(dy_of(t), F64).abs()
  mu, var = x.mean(dim=0), x.var(dim=0, unbiased=False)
  s = _stats_bound(xa, x, mu, var, B, False, False)
  r, dev, e_xh = s['r'], s['dev'], s['e_xh']
  mm, mv = _t(t['mm'], F64), _t(t['mv'], F64)
  om = 1.0 - MOM
  bd = dict(save_mean=s['d_mu'], save_invstd=r * s['dr_rel'],
            mm=om * s['d_mu'] + 6 * U * (mm.abs() + om * (mm.abs() + mu.abs())),
            mv=om * s['d_var'] + 6 * U * (mv.abs() + om * (mv.abs() + var)))
  p = torch.sigmoid((x - mu) * r)
  dp = p * (1 - p) * (e_xh + EXP_U * U) + 4 * U * p + FLT_MIN
  bd['y'] = (aa + 1) * xa * dp + 8 * U * (aa * (1 + p) * xa + p * xa)
  d_direct = dya * (1 + aa) * dp + 8 * U * dya * (aa + (1 + aa) * p)
  Mq = dya * xa * (1 + aa) * p * (1 + p)
  d_q = dya * xa * (1 + aa) * (dp * (1 + p) + p * (dp + 2 * U * (1 + p))) + 10 * U * Mq
  through, _, _, Asg, Asgx = _dx_bound(Mq, d_q, r * dev, e_xh, r, s['dr_rel'], torch.ones_like(r), B)
  M_through = r * (Mq + Asg / B + r * dev * Asgx / B)
  bd['dx'] = d_direct + through + 2 * U * (dya * (aa + (1 + aa) * p) + M_through)
  bd['dalpha'] = (dya * xa * (dp + 2 * U * (1 + p))).sum(dim=0) + (B + 4) * U * (dya * (1 + p) * xa).sum(dim=0)
  return bd


# ------------------------------------------------------------------------------------------------------------------
# runners (be: RefBackend, a planted-mistake subclass, or HipBackend)
# ------------------------------------------------------------------------------------------------------------------
def _dev(v, dev):
  return None if v is None else v.to(dev)


def run_bn(be, t, mode, act, dev='cpu', fwd=None):
  """fwd: (y, mean, invstd, mm, mv) already produced by a fused form; otherwise be.bn_act_fwd.  Then the backward,
  fresh buffers and accumulate-into, chained from that forward."""
  x, b, gamma, beta = (_dev(t[k], dev) for k in ('x', 'bias', 'gamma', 'beta'))
  res = {}
  if fwd is None:
    mm, mv = (t['mm'].to(dev).clone(), t['mv'].to(dev).clone()) if mode != BN_NONE else (None, None)
    y, mean, invstd = be.bn_act_fwd(x, b, gamma, beta, mode, EPS, MOM, mm, mv, act)
  else:
    y, mean, invstd, mm, mv = fwd
  res['y'] = y
  if mode != BN_NONE:
    res.update(save_mean=mean, save_invstd=invstd, mm=mm, mv=mv)
  dy = dy_of(t, dev)
  need_bias, need_affine = b is not None, gamma is not None
  dx, dbias, dgamma, dbeta = be.bn_act_bwd(x, b, gamma, y, mean, invstd, dy, mode, act, need_bias, need_affine)
  res['dx'] = dx
  into = [t['old'][k].to(dev).clone() if need else None
          for k, need in (('dbias', need_bias), ('dgamma', need_affine), ('dbeta', need_affine))]
  dx2, _, _, _ = be.bn_act_bwd(x, b, gamma, y, mean, invstd, dy, mode, act, need_bias, need_affine, into=tuple(into))
  assert torch.equal(dx2, dx)
  for name, fresh, acc in (('dbias', dbias, into[0]), ('dgamma', dgamma, into[1]), ('dbeta', dbeta, into[2])):
    if acc is not None:
      res[name], res['acc_' + name] = fresh, acc
  return res


def run_dice(be, t, dev='cpu'):
  x, alpha = t['x'].to(dev), t['alpha'].to(dev)
  mm, mv = t['mm'].to(dev).clone(), t['mv'].to(dev).clone()
  y, mean, invstd = be.dice_fwd(x, alpha, EPS, MOM, mm, mv)
  dx, dalpha = be.dice_bwd(x, alpha, mean, invstd, dy_of(t, dev).contiguous())
  return dict(y=y, save_mean=mean, save_invstd=invstd, mm=mm, mv=mv, dx=dx, dalpha=dalpha)


# ------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------
_MODE = {BN_NONE: 'none', BN_BATCH: 'train', BN_FROZEN: 'frozen'}


def _case(B, N, mode=BN_BATCH, act=ACT_RELU, data='randn', head=64, bias=True, affine=True, dy_wide=False, tag=''):
  affine = affine and mode != BN_NONE  # (gamma and beta belong to the normalisation)
  cid = 'bn-%dx%d-%s-%s-%s%s%s%s%s' % (B, N, _MODE[mode], 'relu' if act else 'lin', data, '' if bias else '-nobias',
                                        '' if affine or mode == BN_NONE else '-noaffine', '-dyld' if dy_wide else '', tag)
  return dict(id=cid, B=B, N=N, mode=mode, act=act, data=data, head=head, bias=bias, affine=affine, dy_wide=dy_wide)


def _bn_cases():
  cs = []
  # shape edges: every B against every N with batch statistics; B = 1 is variance 0, r = 1 / sqrt(eps)
  for B in (1, 2, 15, 16, 17, 33):
    for N in (1, 3, 63, 64, 65, 130):
      cs.append(_case(B, N, dy_wide=N in (3, 64)))
  for B, N in ((1, 3), (17, 65), (33, 130), (16, 64)):
    cs.append(_case(B, N, mode=BN_FROZEN, dy_wide=B == 17))
    cs.append(_case(B, N, mode=BN_NONE, dy_wide=B == 17))
  cs.append(_case(33, 65, act=ACT_NONE))
  cs.append(_case(33, 65, bias=False, affine=False))
  cs.append(_case(33, 65, mode=BN_NONE, bias=False, affine=False))
  # data edges at the smallest shape with more than one row lane trip, batch statistics and frozen
  for data in ('mean1000', 'bigbias', 'const', 'drift', 'mixed'):
    for mode in (BN_BATCH, BN_FROZEN):
      cs.append(_case(33, 5, mode=mode, data=data))
  cs.append(_case(33, 5, data='head0', head=4))
  # 64 row chunks of 32 rows for the stand-alone kernels: the first chunk (and so the pooling pivot of lane group 0) at
  # mean 0, every other row at 1000 +- 1; the same with the drift
  assert choose_chunks(2048, 64) == 64 and rows_per_chunk(2048, 64) == 32
  cs.append(_case(2048, 64, data='head0', head=32))
  cs.append(_case(2048, 64, data='drift'))
  cs.append(_case(2048, 64, data='mean1000'))
  # the last row chunk is EMPTY: 64 chunks of 63 rows cover 4032 >= 3969 with chunk 63 starting at row 3969.  (The stand-alone
  # kernels keep their partial records in the library's own scratch, so the emitted counts cannot be summed here - that is
  # asserted for the contraction-emitted records; what this case shows is that an empty (0, 0, 0) record joins the merge
  # without moving the result, and er_bn_row_chunks(3969, 1000) == 64 is asserted against the library.)
  assert choose_chunks(3969, 1000) == 64 and rows_per_chunk(3969, 1000) == 63 and 63 * 63 == 3969
  cs.append(_case(3969, 1000))
  # more than kInlineChunks partials: the pre-merge launch; tiles_per_block 4 on the scalar (N = 5) and 16-byte (N = 8) lanes
  assert choose_chunks(8225, 5) == 258 > K_INLINE_CHUNKS and choose_chunks(8225, 8) == 258
  cs.append(_case(8225, 5))
  cs.append(_case(8225, 8, data='mean1000'))
  assert choose_chunks(8192, 8) == 256 and apply_tiles_per_block(8192) == 4 and apply_tiles_per_block(8191) == 1
  cs.append(_case(8192, 8))
  cs.append(_case(8192, 5, dy_wide=True))
  cs.append(_case(8192, 8, mode=BN_FROZEN))
  assert apply_tiles_per_block(32769) == 16 and apply_tiles_per_block(32768) == 4
  cs.append(_case(32769, 8))
  cs.append(_case(32769, 5))
  return cs


BN_CASES = _bn_cases()
DICE_CASES = [dict(id='dice-%dx%d-%s' % (B, N, data), B=B, N=N, data=data, head=head) for B, N, data, head in (
    (1, 3, 'randn', 0), (2, 1, 'randn', 0), (17, 65, 'randn', 0), (33, 130, 'randn', 0), (600, 20, 'randn', 0),
    (33, 5, 'mean1000', 0), (33, 5, 'const', 0), (33, 5, 'drift', 0), (33, 5, 'mixed', 0), (2048, 64, 'head0', 32),
    (8225, 5, 'randn', 0))]
LARGE_MEAN_CASE = 'bn-33x5-train-relu-mean1000'


def bn_case(cid):
  return next(c for c in BN_CASES if c['id'] == cid)


@functools.lru_cache(maxsize=None)
def bn_inputs(cid):
  c = bn_case(cid)
  return bn_tensors(cid, c['B'], c['N'], c['data'], c['head'], c['bias'], c['affine'], c['dy_wide'], c['mode'])


@functools.lru_cache(maxsize=None)
def bn_forward_reference(cid):
  """(fp64 forward outputs, graph) of a case: computed once, shared, never written to."""
  c = bn_case(cid)
  return bn_forward(bn_inputs(cid), c['mode'], c['act'], F64)


def bn_reference(cid, y_given):
  """fp64 reference and bound of a case for a backend whose forward produced y_given."""
  c, t = bn_case(cid), bn_inputs(cid)
  fwd, graph = bn_forward_reference(cid)
  want = dict(fwd)
  want.update(bn_backward(t, c['mode'], c['act'], F64, graph, y_given))
  return want, bn_bound(t, c['mode'], c['act'], y_given)


def dice_case(cid):
  return next(c for c in DICE_CASES if c['id'] == cid)


@functools.lru_cache(maxsize=None)
def dice_reference(cid):
  c = dice_case(cid)
  t = bn_tensors(cid, c['B'], c['N'], c['data'], c['head'], bias=False)
  return t, dice_plain(t, F64), {k: v.detach() for k, v in dice_bound(t).items()}


def bn_reference_of(t, mode, act, y_given):
  """fp64 reference and bound for tensors built on the spot (a fused form: x is what its contraction wrote, as data)."""
  fwd, graph = bn_forward(t, mode, act, F64)
  want = dict(fwd)
  want.update(bn_backward(t, mode, act, F64, graph, y_given))
  return want, bn_bound(t, mode, act, y_given), graph['pre'].detach()


def pooled_stats(col_stats, T, N):
  """The (count, mean, M2) records [T, N, 3] a contraction's epilogue emitted, pooled exactly (fp64) -> count, mean, var."""
  st = col_stats.detach().to('cpu', F64)[:T * N * 3].reshape(T, N, 3)
  n = st[:, :, 0].sum(dim=0)
  mean = (st[:, :, 0] * st[:, :, 1]).sum(dim=0) / n
  m2 = (st[:, :, 2] + st[:, :, 0] * (st[:, :, 1] - mean)**2).sum(dim=0)
  return n, mean, m2 / n


def gemm_operands(kind, M, K, N, seed):
  """a [M, K], w [K, N] (float32, CPU) whose product carries a data edge: column 0 of a is the carrier (1, or 0 in the
  first 64-row tile for 'head0', or a ramp for 'drift') and row 0 of w its height."""
  g = torch.Generator().manual_seed(seed)
  a = torch.randn(M, K, generator=g, dtype=F32)
  w = torch.randn(K, N, generator=g, dtype=F32) * (1.0 / K**0.5)
  if kind == 'randn':
    return a, w
  a[:, 0] = 1.0
  w[0] = 1000.0
  if kind == 'head0':
    a[:GEMM_BM, 0] = 0.0
  elif kind == 'drift':
    a[:, 0] = torch.linspace(0, 1, M, dtype=F32)
  else:
    assert kind == 'mean1000', kind
  return a, w


def gemm_bound(a, w, bias=None):
  """|a| . |w| (+ |bias|) times (K + 4) U: a K-term float32 contraction in any order, with a bias addition."""
  a, w = _t(a, F64).cpu(), _t(w, F64).cpu()
  K = a.shape[1]
  ref = a @ w
  M = a.abs() @ w.abs()
  if bias is not None:
    ref, M = ref + _t(bias, F64).cpu(), M + _t(bias, F64).cpu().abs()
  return ref, (K + 4) * U * M


# (M, K, N, kind, flavour) of the contractions whose epilogue emits the statistics: flavour False = f32, 'staged' = bf16 operands
# rounded while staged (both through tile_col_stats), True = the bf16-NT kernel, which has statistics code of its own.
# d_var grows with B (the 2 d_mu mean(dev) term), so a large-mean column tells a float32 E[z^2] - mean^2 from a sound
# evaluation only at small M: every flavour meets 'mean1000' at M <= 130 (naive_tile_stats shows it on the CPU); the
# M = 4096 / 16385 / 32769 cases are there for the paths (merge launch, row tiles per workgroup), not for that.
STATS_FORM_CASES = [
    (4096, 16, 64, 'randn', False), (4096, 16, 64, 'mean1000', False), (4096, 16, 64, 'head0', False), (4096, 16, 64, 'drift', False),
    (130, 7, 65, 'mean1000', False), (33, 5, 3, 'randn', False), (1, 4, 5, 'randn', False),
    (16385, 8, 8, 'head0', False), (16385, 8, 5, 'randn', False),     # 257 row tiles: the merge launch, 4 row tiles per workgroup
    (32769, 4, 8, 'mean1000', False),                                  # 16 row tiles per workgroup, 16-byte lanes
    (4096, 16, 64, 'mean1000', True), (4096, 16, 64, 'head0', True), (130, 8, 72, 'randn', True), (16385, 8, 8, 'drift', True),
    (130, 8, 72, 'mean1000', True), (130, 8, 72, 'head0', True), (33, 8, 8, 'mean1000', True),
    (4096, 16, 64, 'mean1000', 'staged'), (130, 7, 65, 'head0', 'staged'), (16385, 8, 5, 'drift', 'staged'),
    (130, 7, 65, 'mean1000', 'staged')]
STATS_FLAVOUR = {False: 'f32', True: 'bf16nt', 'staged': 'bf16'}


def stats_form_operands(M, K, N, kind):
  a, w = gemm_operands(kind, M, K, N, M + K + N)
  return a, w, torch.randn(N, generator=torch.Generator().manual_seed(N))


def naive_tile_stats(z, naive):
  """(count, mean, M2) per 64-row tile of z in float32, [T * N * 3]: M2 two-pass, or - naive - n (E[z^2] - mean^2), the
  evaluation the emitted-statistics cases must tell apart."""
  z = z.to(F32)
  recs = []
  for r0 in range(0, z.shape[0], GEMM_BM):
    rows = z[r0:r0 + GEMM_BM]
    n = float(rows.shape[0])
    mean = rows.sum(dim=0) / n
    m2 = ((rows * rows).sum(dim=0) / n - mean * mean) * n if naive else ((rows - mean)**2).sum(dim=0)
    recs.append(torch.stack([torch.full_like(mean, n), mean, m2], dim=1))
  return torch.stack(recs).reshape(-1)
