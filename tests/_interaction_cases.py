"""Cases, fp64 references and derived error bounds for the interaction kernels (FM / row sum, DCN cross v1 and the
cross v2 epilogue, DIN concat and pool, MMoE mixing, sigmoid cross-entropy, the four CIN kernels one by one, the DLRM
dot interaction).  No backend is imported here: the CPU
tests (test_interaction_restatement.py) and the GPU tests (test_interaction_gpu.py) hand one to the run_* functions.

Reference.  Every *_formula below is the published formula as the reference project's model code states it, written
with differentiable torch ops and evaluated in torch.float64; every gradient is torch.autograd of that formula (no
hand-written derivative).  The same function evaluated in torch.float32 is the "plain float32" evaluation the CPU
tests hold to half of each bound.  Inputs are float32 values, so the fp64 evaluation starts from exactly the numbers
the kernels read; scalars a kernel takes as a C float (diag, scale, loss_scale) are rounded to float32 in the case.

Bound.  Per element, bound = (n + c) * U * M + floor, with U = 2**-24 the unit roundoff of float32:
  * every float32 operation returns exact * (1 + delta), |delta| <= U.  A result that is a polynomial of the inputs is
    therefore the sum of its monomials, each times at most `depth` factors (1 + delta), depth = the number of
    operations between the monomial's operands and the result; the error is at most depth * U * (sum of the monomials'
    absolute values) to first order.  n + c is that depth: n the accumulation chain (F, d, L, E, H, T, B ...), c the
    elementwise operations around it.  Any summation order has a chain of at most n - 1 additions, so the bound holds
    for the kernels' wave reductions, for torch's pairwise sums and for the oracle alike.
  * M is that sum of absolute monomials: the formula with every term replaced by its absolute value and every
    subtraction by an addition (*_abs below).  The gradient's M is autograd of the SAME abs formula with |dout|: the
    derivative of a polynomial with non-negative coefficients at non-negative points is the sum of the absolute values
    of the gradient's monomials.
  * expf / log1pf are taken at the OpenCL full-profile accuracy (3 ulp and 2 ulp; an ulp is 2 U), the most any
    conforming device library may err; softmax adds the relative error |argument error| that exp passes on, see
    _softmax_bound.
  * floor = FLT_MIN (2**-126) times whatever multiplies an exp result: values below FLT_MIN may be flushed to zero.
  * second-order terms are below n * U of the first-order ones (n * U <= 3e-3 for every case here) and are covered by
    counting n where n - 1 would do.
  * c is TWICE the number of elementwise operations on the longest path: an elementwise operation is held to faithful
    rounding (one of the two neighbouring floats, below 1 ulp = 2 U), not to round-to-nearest (U).  A bound at the exact
    round-to-nearest worst case is reached, ratio 1, by a correct evaluation of a one-operation result; with 2 U per
    operation a round-to-nearest evaluation sits at half the bound or below - which is what the plain float32 test
    asserts - and one wrong bit still shows.  The chain n is counted once: its roundings do not all align.
A bound of exactly 0 (copies, masked positions, columns beside a strided destination) demands equality.
"""
import functools

import numpy as np
import torch

U = 2.0**-24
FLT_MIN = 2.0**-126
EXP_U = 6  # expf within 3 ulp = 6 U
LOG_U = 4  # log1pf within 2 ulp = 4 U
F64, F32 = torch.float64, torch.float32


def f32(v):
  """A python scalar rounded to the float32 the C ABI carries."""
  return float(np.float32(v))


def _gen(seed):
  return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
  return torch.randn(*shape, generator=g, dtype=F32)


def _t(x, dt):
  return x.detach().to(dt)


def _grads(out, wrt, dout):
  return torch.autograd.grad(out, wrt, dout, retain_graph=True, allow_unused=True)


# ------------------------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------------------------
def ratio(got, ref, bound):
  """max |got - ref| / bound over the tensor; inf where the bound is 0 and the values differ, nan -> inf."""
  got = got.detach().to('cpu', F64).reshape(ref.shape)
  diff = (got - ref).abs()
  r = torch.where(bound > 0, diff / bound.clamp_min(1e-300), torch.where(diff == 0, torch.zeros_like(diff),
                                                                        torch.full_like(diff, float('inf'))))
  r = torch.where(torch.isnan(r), torch.full_like(r, float('inf')), r)
  return float(r.max()) if r.numel() else 0.0


def ratios(got, ref, bound):
  assert set(got) == set(ref) == set(bound), (sorted(got), sorted(ref), sorted(bound))
  return {k: ratio(got[k], ref[k], bound[k]) for k in sorted(ref)}


def check(who, op, case, got, ref, bound, frac=1.0):
  """Print every error-to-bound ratio, then assert each is at most `frac`."""
  rs = ratios(got, ref, bound)
  for k, v in rs.items():
    print('RATIO who=%s op=%s case=%s tensor=%s ratio=%.4g' % (who, op, case['id'], k, v))
  bad = {k: v for k, v in rs.items() if not v <= frac}
  assert not bad, '%s %s %s: error / bound above %g: %s' % (who, op, case['id'], frac, bad)
  return rs


# ------------------------------------------------------------------------------------------------------------------
# FM and the row sum:  fm = 0.5 * ((sum_f e)^2 - sum_f e^2),  rowsum = sum_j x_j
# ------------------------------------------------------------------------------------------------------------------
# layouts of x: 'contig'; 'wide' = the first F*D columns of a wider matrix (x_stride > F*D, base aligned);
# 'off1' = a view that starts one column in (base 4 bytes off a 16-byte boundary: fm_fwd_kernel<4> must give way to <1>)
FM_PAD = 8   # extra columns of the wider matrix (a multiple of 4: 'wide' keeps the <4> kernel when D % 4 == 0)
FM_INTO_OFF, FM_INTO_PAD = 2, 5  # into= is columns [2, 2 + F*D) of a [B, F*D + 5] buffer: strided, misaligned


def _fm_cases():
  cases = []
  for B, F, D in ((513, 39, 16), (7, 3, 5), (64, 8, 64)):
    # (513, 39, 16): DeepFM's fields, three 16-field trips and more than one block; (7, 3, 5): D % 4 != 0 -> <1>;
    # (64, 8, 64): F below one trip
    for layout in ('contig', 'wide', 'off1'):
      cases.append(dict(id='fm-%dx%dx%d-%s' % (B, F, D, layout), B=B, F=F, D=D, layout=layout, offset=0.0))
  # field vectors with a common offset of 100: S^2 and sum e^2 are both ~1e5 times the spread that carries the signal
  cases.append(dict(id='fm-64x8x64-contig-offset100', B=64, F=8, D=64, layout='contig', offset=100.0))
  return cases


FM_CASES = _fm_cases()


def fm_vec_expected(case):
  """er_fm_fwd's rule: D % 4 == 0, x_stride % 4 == 0, 16-byte aligned base."""
  return case['D'] % 4 == 0 and case['layout'] in ('contig', 'wide')


def fm_view(xw, case):
  n = case['F'] * case['D']
  return {'contig': xw, 'wide': xw[:, :n], 'off1': xw[:, 1:1 + n]}[case['layout']]


def fm_inputs(case):
  g = _gen(11)
  B, n, D = case['B'], case['F'] * case['D'], case['D']
  W = n if case['layout'] == 'contig' else n + FM_PAD
  xw = _randn(g, B, W) + case['offset']
  return dict(xw=xw, g=_randn(g, B, D), gs=_randn(g, B, 1), old=_randn(g, B, n + FM_INTO_PAD))


def _fm(e):
  S = e.sum(dim=1)
  return 0.5 * (S * S - (e * e).sum(dim=1)), S


def _fm_abs(e):
  A = e.sum(dim=1)
  return 0.5 * (A * A + (e * e).sum(dim=1)), A


def fm_formula(case, inp, dt):
  B, F, D = case['B'], case['F'], case['D']
  x = _t(fm_view(inp['xw'], case), dt).contiguous().requires_grad_(True)
  fm, S = _fm(x.reshape(B, F, D))
  rs = x.sum(dim=1, keepdim=True)
  dx_fm, = _grads(fm, x, _t(inp['g'], dt))
  dx_rs, = _grads(rs, x, _t(inp['gs'], dt))
  old = _t(inp['old'], dt)
  acc_fm, acc_rs = old.clone(), old.clone()
  sl = slice(FM_INTO_OFF, FM_INTO_OFF + F * D)
  acc_fm[:, sl] += dx_fm
  acc_rs[:, sl] += dx_rs
  return dict(fm=fm, S=S, rowsum=rs, dx_fm=dx_fm, dx_rs=dx_rs, acc_fm=acc_fm, acc_rs=acc_rs)


def fm_bound(case, inp):
  B, F, D = case['B'], case['F'], case['D']
  n = F * D
  xa = _t(fm_view(inp['xw'], case), F64).abs().contiguous().requires_grad_(True)
  ga, gsa, olda = _t(inp['g'], F64).abs(), _t(inp['gs'], F64).abs(), _t(inp['old'], F64).abs()
  Mfm, A = _fm_abs(xa.reshape(B, F, D))
  Mdx, = _grads(Mfm, xa, ga)  # = |g| * (A + |e|)
  sl = slice(FM_INTO_OFF, FM_INTO_OFF + n)
  b = {}
  # S: F - 1 additions.  n = F, c = 0.
  b['S'] = F * U * A
  # fm: S carries (F - 1) U A and enters the square twice (d(S^2) = 2 S dS, |S| <= A), the square rounds once;
  # each e^2 rounds once and their sum F - 1 times; one subtraction; * 0.5 is exact:
  #   0.5 U (2 F A^2 + (F + 1) Q) <= (2 F + 1) U M with M = 0.5 (A^2 + Q).  n = 2 F (the chain, twice), two
  # elementwise operations on the path (a square, the subtraction): c = 4.
  b['fm'] = (2 * F + 4) * U * Mfm
  # rowsum: F*D - 1 additions.  n = F*D, c = 0.
  b['rowsum'] = n * U * xa.sum(dim=1, keepdim=True)
  # dx = g * (S - e) on the SAVED float32 S: S's chain F, the subtraction, the product.  n = F, c = 4.
  b['dx_fm'] = (F + 4) * U * Mdx
  # the row sum's gradient is a broadcast copy of g
  b['dx_rs'] = torch.zeros(B, n, dtype=F64)
  # accumulate=True into a strided slice: one more addition, old joins M; the columns beside the slice must not move
  b['acc_fm'] = torch.zeros(B, n + FM_INTO_PAD, dtype=F64)
  b['acc_fm'][:, sl] = (F + 6) * U * (Mdx + olda[:, sl])
  b['acc_rs'] = torch.zeros(B, n + FM_INTO_PAD, dtype=F64)
  b['acc_rs'][:, sl] = 2 * U * (gsa + olda[:, sl])  # one addition.  c = 2.
  return {k: v.detach() for k, v in b.items()}


def run_fm(be, case, inp, dev, seen=None):
  F, D = case['F'], case['D']
  n = F * D
  x = fm_view(inp['xw'].to(dev), case)
  g, gs = inp['g'].to(dev), inp['gs'].to(dev)
  if seen is not None:  # what er_fm_fwd's choice between <4> and <1> looks at
    seen.update(x_ptr=x.data_ptr(), x_stride=x.stride(0))
  fm, S = be.fm_fwd(x, F, D)
  rs = be.rowsum_fwd(x, n)
  dx_fm = be.fm_bwd(x, S, g, F, D)
  dx_rs = be.rowsum_bwd(gs, n)
  acc_fm, acc_rs = inp['old'].to(dev).clone(), inp['old'].to(dev).clone()
  be.fm_bwd(x, S, g, F, D, into=acc_fm[:, FM_INTO_OFF:FM_INTO_OFF + n], accumulate=True)
  be.rowsum_bwd(gs, n, into=acc_rs[:, FM_INTO_OFF:FM_INTO_OFF + n], accumulate=True)
  return dict(fm=fm, S=S, rowsum=rs, dx_fm=dx_fm, dx_rs=dx_rs, acc_fm=acc_fm, acc_rs=acc_rs)


# ------------------------------------------------------------------------------------------------------------------
# DCN cross v1:  x_{l+1} = x0 * (x_l . w_l) + b_l + x_l
# ------------------------------------------------------------------------------------------------------------------
CROSS_V1_CASES = [
    dict(id='v1-130x70x3', B=130, d=70, L=3),      # the ordinary shape: two 64-column register slots, d % 64 != 0
    dict(id='v1-1100x70x2', B=1100, d=70, L=2),    # er_cross_v1_bwd_partials caps the grid at 512: r += gridDim.x trips 3 times
    dict(id='v1-3x1024x2', B=3, d=1024, L=2),      # d = 64 * kCrossE fills the register-resident row
    dict(id='v1-3x1024x9', B=3, d=1024, L=9),      # 2*L*d*4 = 72 KB of LDS: past the 64 KB hipFuncSetAttribute branch
    dict(id='v1-2x1024x20', B=2, d=1024, L=20),    # exactly the 160 KB that ER_REQUIRE admits
    dict(id='v1-5x17x1', B=5, d=17, L=1),          # the small case: one layer, a quarter of a wave
]
# refused: d past the register row; L * d one float past the LDS accumulators (20481 = 3 * 6827)
CROSS_V1_REFUSED = [dict(id='v1-refuse-d1025', B=2, d=1025, L=1), dict(id='v1-refuse-Ld20481', B=2, d=3, L=6827)]


def cross_v1_inputs(case):
  g = _gen(12)
  B, d, L = case['B'], case['d'], case['L']
  # |w| ~ 1 / (d sqrt(L)) keeps the ABS recurrence (M) within ~10x of the values over 20 layers of d = 1024
  return dict(x0=_randn(g, B, d), w=_randn(g, L, d) / (d * L**0.5), b=0.1 * _randn(g, L, d), dout=_randn(g, B, d))


def _cross_v1(x0, w, b):  # all-positive coefficients: it is its own abs formula on abs inputs
  x, dots = x0, []
  for l in range(w.shape[0]):
    dot = (x * w[l]).sum(dim=1, keepdim=True)
    dots.append(dot)
    x = x0 * dot + b[l] + x
  return x, torch.cat(dots, dim=1)


def _cross_v1_eval(x0, w, b, dout):
  x0, w, b = (t.requires_grad_(True) for t in (x0, w, b))
  out, dots = _cross_v1(x0, w, b)
  dx0, dw, db = _grads(out, (x0, w, b), dout)
  return dict(out=out, dots=dots, dx0=dx0, dw=dw, db=db)


def cross_v1_formula(case, inp, dt):
  return _cross_v1_eval(*(_t(inp[k], dt) for k in ('x0', 'w', 'b', 'dout')))


def cross_v1_bound(case, inp):
  B, d, L = case['B'], case['d'], case['L']
  M = _cross_v1_eval(*(_t(inp[k], F64).abs() for k in ('x0', 'w', 'b', 'dout')))
  # one layer: a d-term dot (d - 1 additions + the product), then product, two additions: depth d + 3.
  # out / dots after L layers: n = L * d, c = 6 L.
  fwd = L * (d + 6) * U
  # backward: x_l recomputed from the saved dots (L (d + 3)), the gradient's own recurrence through L layers, each a
  # d-term dot and three elementwise operations (L (d + 3)), B rows summed into dw / db (B) or L layer terms into dx0
  # (L), two more products.  n = 2 L d + B + L, c = 12 L + 4.
  bwd = (2 * L * (d + 6) + B + L + 4) * U
  return dict(out=fwd * M['out'], dots=fwd * M['dots'], dx0=bwd * M['dx0'], dw=bwd * M['dw'], db=bwd * M['db'])


def run_cross_v1(be, case, inp, dev, seen=None):
  x0, w, b, dout = (inp[k].to(dev) for k in ('x0', 'w', 'b', 'dout'))
  out, dots = be.cross_v1_fwd(x0, w, b)
  dx0, dw, db = be.cross_v1_bwd(x0, w, b, dots, dout)
  return dict(out=out, dots=dots, dx0=dx0, dw=dw, db=db)


# ------------------------------------------------------------------------------------------------------------------
# DCN cross v2 epilogue:  out = x0 * (u + bias + diag * x) + x
# ------------------------------------------------------------------------------------------------------------------
# layouts of the three strided operands (dout, dx0, dx), each columns [off, off + d) of a [B, ld] buffer:
#   'contig' ld = d;  'ld4' ld % 4 == 0 and a 16-byte aligned base;  'ldodd' ld % 4 != 0;  'off1' base one column in
CROSS_V2_SHAPES = [(77, 130), (5, 128), (9, 3)]  # d % 4 != 0 over several blocks; d % 4 == 0 (<4> eligible); tiny
CROSS_V2_LAYOUTS = ('contig', 'ld4', 'ldodd', 'off1')
CROSS_V2_CASES = [dict(id='v2-%dx%d-%s' % (B, d, lay), B=B, d=d, layout=lay) for B, d in CROSS_V2_SHAPES
                  for lay in CROSS_V2_LAYOUTS]
CROSS_V2_DIAGS = (0.0, f32(0.3))


def cross_v2_variants():
  """(diag, bias present, dx given, acc0, accx): accx has no meaning without dx."""
  for diag in CROSS_V2_DIAGS:
    for has_bias in (True, False):
      for has_dx in (True, False):
        for acc0 in (0, 1):
          for accx in ((0, 1) if has_dx else (0,)):
            yield diag, has_bias, has_dx, acc0, accx


def cross_v2_layout(case):
  d = case['d']
  r4 = (d + 3) // 4 * 4
  return {'contig': (d, 0), 'ld4': (r4 + 8, 4), 'ldodd': (r4 + 9, 4), 'off1': (r4 + 8, 1)}[case['layout']]


def cross_v2_vec_expected(case):
  """er_cross_v2_epilogue_bwd_acc's rule: d % 4 == 0, the three leading dimensions % 4 == 0, every base 16-byte aligned."""
  return case['d'] % 4 == 0 and case['layout'] in ('contig', 'ld4')


def cross_v2_inputs(case):
  g = _gen(13)
  B, d = case['B'], case['d']
  ld, _ = cross_v2_layout(case)
  return dict(x0=_randn(g, B, d), x=_randn(g, B, d), u=_randn(g, B, d), bias=_randn(g, d), gbuf=_randn(g, B, ld),
              old0=_randn(g, B, ld), oldx=_randn(g, B, ld))


def _cross_v2(x0, x, u, bias, diag):  # all-positive coefficients: its own abs formula on abs inputs
  t = u if bias is None else u + bias
  if diag != 0:
    t = t + diag * x
  return x0 * t + x


def _cross_v2_eval(case, inp, dt, variant, absolute):
  diag, has_bias, has_dx, acc0, accx = variant
  ld, off = cross_v2_layout(case)
  sl = slice(off, off + case['d'])
  c = (lambda k: _t(inp[k], dt).abs()) if absolute else (lambda k: _t(inp[k], dt))
  x0 = c('x0').requires_grad_(True)
  u = c('u').requires_grad_(True)
  bias = c('bias') if has_bias else None
  dout = c('gbuf')[:, sl]
  if has_dx:
    x = c('x').requires_grad_(True)
    out = _cross_v2(x0, x, u, bias, diag)
    g0, gx, du = _grads(out, (x0, x, u), dout)
  else:  # the first layer of a stack: x IS x0, and its gradient joins dx0
    out = _cross_v2(x0, x0, u, bias, diag)
    g0, du = _grads(out, (x0, u), dout)
    gx = None
  old0, oldx = c('old0'), c('oldx')
  dx0 = old0.clone()
  dx0[:, sl] = (old0[:, sl] + g0) if acc0 else g0
  r = dict(out=out, du=du, dx0=dx0)
  if has_dx:
    dx = oldx.clone()
    dx[:, sl] = (oldx[:, sl] + gx) if accx else gx
    r['dx'] = dx
  return {k: v.detach() for k, v in r.items()}


def cross_v2_formula(case, inp, dt, variant):
  return _cross_v2_eval(case, inp, dt, variant, False)


def cross_v2_bound(case, inp, variant):
  _, off = cross_v2_layout(case)
  sl = slice(off, off + case['d'])
  M = _cross_v2_eval(case, inp, F64, variant, True)
  b = {}
  # out: u + bias, diag * x, their sum, the product with x0, + x.  n = 0, c = 10.
  b['out'] = 10 * U * M['out']
  # du = dout * x0.  c = 2.
  b['du'] = 2 * U * M['du']
  # dx0 (+)= dout * t, t three operations deep; without dx the gradient of x (three more) is added to it; one more
  # addition when it accumulates: six operations on the longest path.  c = 12.  Beside the slice nothing may move.
  b['dx0'] = torch.zeros_like(M['dx0'])
  b['dx0'][:, sl] = 12 * U * M['dx0'][:, sl]
  if 'dx' in M:
    # dx (+)= dout + dout * x0 * diag: two products, the addition, the accumulation.  c = 8.
    b['dx'] = torch.zeros_like(M['dx'])
    b['dx'][:, sl] = 8 * U * M['dx'][:, sl]
  return b


def run_cross_v2(be, case, inp, dev, variant, seen=None):
  diag, has_bias, has_dx, acc0, accx = variant
  _, off = cross_v2_layout(case)
  sl = slice(off, off + case['d'])
  x0, u = inp['x0'].to(dev), inp['u'].to(dev)
  x = inp['x'].to(dev) if has_dx else x0
  bias = inp['bias'].to(dev) if has_bias else None
  dout = inp['gbuf'].to(dev)[:, sl]
  buf0, bufx = inp['old0'].to(dev).clone(), inp['oldx'].to(dev).clone()
  if seen is not None:  # what er_cross_v2_epilogue_bwd_acc's choice between <4> and <1> looks at
    ts = [x0, x, u, dout, buf0[:, sl]] + ([bias] if has_bias else []) + ([bufx[:, sl]] if has_dx else [])
    seen.update(ptrs=[t.data_ptr() for t in ts], lds=[dout.stride(0), buf0.stride(0)] + ([bufx.stride(0)] if has_dx else []))
  out = be.cross_v2_fwd(x0, x, u, bias, diag)
  du = be.cross_v2_bwd_acc(x0, x, u, bias, diag, dout, buf0[:, sl], acc0, bufx[:, sl] if has_dx else None, accx)
  if seen is not None:
    seen['ptrs'].append(du.data_ptr())
  r = dict(out=out, du=du, dx0=buf0)
  if has_dx:
    r['dx'] = bufx
  return r


def cross_v2_plain_formula(case, inp, dt, diag, has_bias):
  x0, x, u = (_t(inp[k], dt).requires_grad_(True) for k in ('x0', 'x', 'u'))
  out = _cross_v2(x0, x, u, _t(inp['bias'], dt) if has_bias else None, diag)
  _, off = cross_v2_layout(case)
  dx0, dx, du = _grads(out, (x0, x, u), _t(inp['gbuf'], dt)[:, off:off + case['d']])
  return dict(dx0=dx0, dx=dx, du=du)


def cross_v2_plain_bound(case, inp, diag, has_bias):
  a = {k: v.abs() for k, v in inp.items()}
  M = cross_v2_plain_formula(case, a, F64, diag, has_bias)
  # dx0 = dout * t (4 operations: c = 8), dx = dout + dout * x0 * diag (3: c = 6), du = dout * x0 (1: c = 2)
  return dict(dx0=8 * U * M['dx0'], dx=6 * U * M['dx'], du=2 * U * M['du'])


def run_cross_v2_plain(be, case, inp, dev, diag, has_bias):
  _, off = cross_v2_layout(case)
  x0, x, u = (inp[k].to(dev) for k in ('x0', 'x', 'u'))
  dout = inp['gbuf'].to(dev)[:, off:off + case['d']].contiguous()
  dx0, dx, du = be.cross_v2_bwd(x0, x, u, inp['bias'].to(dev) if has_bias else None, diag, dout)
  return dict(dx0=dx0, dx=dx, du=du)


# ------------------------------------------------------------------------------------------------------------------
# softmax: shared by DIN pool and MMoE
# ------------------------------------------------------------------------------------------------------------------
def _softmax_bound(s, arg_err, n):
  """Per-element bound of p = softmax(s) over the last axis (n entries).  s: the exact arguments (fp64); arg_err: the
  absolute error, in units of U, each argument already carries when the maximum is subtracted (2 |s| for a rounded
  product, 0 for an input or a constant).
    e_t = expf(s_t - mx): the subtraction rounds (2 |s_t - mx| U), s_t and mx bring arg_err; an absolute error of the
          argument is a relative error of exp; expf itself EXP_U.   rel(e_t) = (2 |s_t - mx| + err_t + err_mx + EXP_U) U
    den = sum e_t, all positive, n - 1 additions:                    rel(den) = sum_j p_j rel(e_j) + n U
    p_t = e_t / den, one division:                                   rel(p_t) = rel(e_t) + rel(den) + 2 U
  -> bound = p_t * rel(p_t) + FLT_MIN (a probability below FLT_MIN may be flushed to zero)."""
  mx, at = s.max(dim=-1, keepdim=True)
  p = torch.softmax(s, dim=-1)
  rel_e = (2 * (s - mx).abs() + arg_err + arg_err.gather(-1, at) + EXP_U) * U
  rel_p = rel_e + (p * rel_e).sum(dim=-1, keepdim=True) + (n + 2) * U
  return p, p * rel_p + FLT_MIN


def _softmax_grad_bound(p, bp, dp, D, n_dp, n_soft, active, scale):
  """Bound of ds_t = p_t * (dp_t - sum_j p_j dp_j) * scale on the float32 p the forward saved.  dp_t is a dot product of
  n_dp terms with sum of absolute terms D_t:  err(dp_t) = n_dp U D_t;
    dot = sum_j p_j dp_j:  err = sum_j (bp_j |dp_j| + p_j err(dp_j)) + (n_soft + 2) U P,   P = sum_j p_j |dp_j|
    the subtraction, the product with p_t and the one with scale: three operations (6 U) on at most |dp_t| + P.
  Positions outside `active` get exactly zero."""
  edp = n_dp * U * D
  P = (p * dp.abs()).sum(dim=-1, keepdim=True)
  edot = (bp * dp.abs() + p * edp).sum(dim=-1, keepdim=True) + (n_soft + 2) * U * P
  span = dp.abs() + P
  b = abs(scale) * (bp * span + p * (edp + edot + 6 * U * span)) + FLT_MIN
  return torch.where(active, b, torch.zeros_like(b))


# ------------------------------------------------------------------------------------------------------------------
# DIN:  concat [q, h, q - h, q * h];  pool softmax(where(t < len, s * scale, -2**32 + 1)) @ hist
# ------------------------------------------------------------------------------------------------------------------
DIN_PAD = float(-2**32 + 1)
DIN_MASKED_FILL = 1e30  # what the masked score positions hold: it must not influence anything
DIN_FAST_SHAPES = [(33, 50, 32), (130, 50, 4), (7, 64, 256), (9, 1, 16)]
# (33, 50, 32): DIN's own shape, C = E/4 = 8 chunks; (130, 50, 4): C = 1 (R = 64 rows a pass), more than one block;
# (7, 64, 256): the extreme C = 64 (R = 1) at L = 64, every lane a position; (9, 1, 16): one position
DIN_GENERAL_SHAPES = [(4, 70, 8), (5, 13, 12), (3, 20, 80)]
# (4, 70, 8): L > 64, positions strided over the lanes; (5, 13, 12): E/4 = 3 is no power of two;
# (3, 20, 80): E > 64 runs the general kernel's `e += 64` loop, E/4 = 20 is no power of two


def din_fast_expected(case):
  """din_fast_ok's shape rule (the alignment half is checked on the tensors, in the GPU test)."""
  L, E = case['L'], case['E']
  C = E // 4
  return L <= 64 and E % 4 == 0 and 1 <= C <= 64 and (C & (C - 1)) == 0


def _din_cases():
  cases = []
  for shapes, path in ((DIN_FAST_SHAPES, 'fast'), (DIN_GENERAL_SHAPES, 'general')):
    for i, (B, L, E) in enumerate(shapes):
      for tag, scale in (('s1', 1.0), ('sE', f32(E**-0.5))):
        cases.append(dict(id='din-%dx%dx%d-%s-%s' % (B, L, E, path, tag), B=B, L=L, E=E, path=path, scale=scale, sat=False))
      if i == 0:  # active scores of +-30: the softmax saturates
        cases.append(dict(id='din-%dx%dx%d-%s-sat' % (B, L, E, path), B=B, L=L, E=E, path=path, scale=1.0, sat=True))
  return cases


DIN_CASES = _din_cases()


def din_inputs(case):
  g = _gen(14)
  B, L, E = case['B'], case['L'], case['E']
  seq_len = torch.randint(0, L + 1, (B,), generator=g, dtype=torch.int32)
  seq_len[0], seq_len[1], seq_len[2] = 0, 1, L  # every case has an empty, a one-item and a full history
  assert {0, 1, L} <= set(seq_len.tolist())
  scores = _randn(g, B, L)
  if case['sat']:
    scores = 30.0 * torch.sign(scores)
  mask = torch.arange(L)[None, :] < seq_len[:, None].to(torch.int64)
  scores = torch.where(mask, scores, torch.full_like(scores, DIN_MASKED_FILL))
  return dict(seq_len=seq_len, mask=mask, scores=scores, hist=_randn(g, B, L, E), q=_randn(g, B, E),
              dout=_randn(g, B, E), dcat=_randn(g, B, L, 4 * E), old=_randn(g, B, L, E))


def din_formula(case, inp, dt):
  scale, mask = case['scale'], inp['mask']
  scores, hist, q = (_t(inp[k], dt).requires_grad_(True) for k in ('scores', 'hist', 'q'))
  s = torch.where(mask, scores * scale, torch.full_like(scores, DIN_PAD))
  p = torch.softmax(s, dim=1)
  out = torch.bmm(p[:, None, :], hist)[:, 0, :]
  dscores, dhist = _grads(out, (scores, hist), _t(inp['dout'], dt))
  qq = q[:, None, :].expand_as(hist)
  cat = torch.cat([qq, hist, qq - hist, qq * hist], dim=-1)
  dq, dh = _grads(cat, (q, hist), _t(inp['dcat'], dt))
  old = _t(inp['old'], dt)
  return dict(probs=p, out=out, dscores=dscores, dhist=dhist, dhist_fresh=dhist, dhist_acc=old + dhist, cat=cat, dq=dq,
              dh=dh, dh_fresh=dh, dh_acc=old + dh)


def din_bound(case, inp):
  B, L, E, scale = case['B'], case['L'], case['E'], case['scale']
  mask = inp['mask']
  scores, hist, q, g, dcat, old = (_t(inp[k], F64) for k in ('scores', 'hist', 'q', 'dout', 'dcat', 'old'))
  s = torch.where(mask, scores * scale, torch.full_like(scores, DIN_PAD))
  # an active argument is the rounded product score * scale (one operation: 2 |s| U); the pad is one constant, the same float32 in every
  # masked position, so a masked argument brings no error of its own
  p, bp = _softmax_bound(s, torch.where(mask, 2 * s.abs(), torch.zeros_like(s)), L)
  ha, ga = hist.abs(), g.abs()
  b = dict(probs=bp)
  # out_e = sum_t p_t h_te on the computed p: bp_t |h_te| each, then a product and L - 1 additions.  n = L, c = 2.
  b['out'] = (bp[:, :, None] * ha).sum(dim=1) + (L + 2) * U * (p[:, :, None] * ha).sum(dim=1)
  # dscores: the softmax gradient over dp_t = sum_e dout_e h_te (n = E, then n = L for the dot with p); masked -> 0
  dp = (hist * g[:, None, :]).sum(dim=-1)
  D = (ha * ga[:, None, :]).sum(dim=-1)
  b['dscores'] = _softmax_grad_bound(p, bp, dp, D, E, L, mask, scale)
  # dhist_te = p_t dout_e: bp_t |dout_e| and one product (c = 2); accumulating adds once more, on |old| + |p dout|
  pg = p[:, :, None] * ga[:, None, :]
  b['dhist'] = bp[:, :, None] * ga[:, None, :] + 2 * U * pg + FLT_MIN
  b['dhist_fresh'] = b['dhist']
  b['dhist_acc'] = b['dhist'] + 2 * U * (old.abs() + pg)
  # concat: q and h are copied (exact); q - h and q * h round once.  c = 2.
  qa = q.abs()[:, None, :].expand_as(ha)
  zero = torch.zeros_like(ha)
  b['cat'] = torch.cat([zero, zero, 2 * U * (qa + ha), 2 * U * qa * ha], dim=-1)
  g0, g1, g2, g3 = (dcat[..., i * E:(i + 1) * E].abs() for i in range(4))
  # dq_e = sum_t (g0 + g2 + g3 h): L terms, each two additions and a product deep.  n = L, c = 6.
  b['dq'] = (L + 6) * U * (g0 + g2 + g3 * ha).sum(dim=1)
  # dh = g1 - g2 + g3 q: three operations, c = 6; accumulating: four, c = 8, on |old| more
  Mdh = g1 + g2 + g3 * qa
  b['dh'] = 6 * U * Mdh
  b['dh_fresh'] = b['dh']
  b['dh_acc'] = 8 * U * (Mdh + old.abs())
  return b


def run_din(be, case, inp, dev, seen=None):
  scale = case['scale']
  scores, hist, q, dout, dcat, seq_len = (inp[k].to(dev) for k in ('scores', 'hist', 'q', 'dout', 'dcat', 'seq_len'))
  out, probs = be.din_pool_fwd(scores, hist, seq_len, scale)
  dscores, dhist = be.din_pool_bwd(probs, hist, seq_len, dout, scale)
  fresh, acc = inp['old'].to(dev).clone(), inp['old'].to(dev).clone()
  ds2, _ = be.din_pool_bwd(probs, hist, seq_len, dout, scale, dhist=fresh, acc_h=False)
  ds3, _ = be.din_pool_bwd(probs, hist, seq_len, dout, scale, dhist=acc, acc_h=True)
  assert torch.equal(ds2, dscores) and torch.equal(ds3, dscores)
  cat = be.din_concat_fwd(q, hist)
  dq, dh = be.din_concat_bwd(q, hist, dcat)
  cfresh, cacc = inp['old'].to(dev).clone(), inp['old'].to(dev).clone()
  dq2, _ = be.din_concat_bwd(q, hist, dcat, dh=cfresh, acc_h=False)
  dq3, _ = be.din_concat_bwd(q, hist, dcat, dh=cacc, acc_h=True)
  assert torch.equal(dq2, dq) and torch.equal(dq3, dq)
  if seen is not None:  # every tensor din_fast_ok's alignment half looks at
    seen.update(ptrs=[t.data_ptr() for t in (hist, out, dout, dhist, fresh, acc, q, dcat, dq, dh, cfresh, cacc)])
  return dict(probs=probs, out=out, dscores=dscores, dhist=dhist, dhist_fresh=fresh, dhist_acc=acc, cat=cat, dq=dq, dh=dh,
              dh_fresh=cfresh, dh_acc=cacc)


# ------------------------------------------------------------------------------------------------------------------
# MMoE mixing:  out[t, b, :] = sum_e softmax(logits[t, b, :])_e * experts[e, b, :]
# ------------------------------------------------------------------------------------------------------------------
MMOE_CASES = [
    dict(id='mmoe-4x5x130x64', T=4, E=5, B=130, H=64, big=False),     # the ordinary shape, H one wave exactly
    dict(id='mmoe-1x1x3x7', T=1, E=1, B=3, H=7, big=False),           # one expert (the gate is 1), H below a wave
    dict(id='mmoe-3x32x9x100', T=3, E=32, B=9, H=100, big=False),     # E = kMaxExperts; H no multiple of 64, two trips
    dict(id='mmoe-2x4x65x33', T=2, E=4, B=65, H=33, big=False),       # odd everything, T*B over a block of waves
    dict(id='mmoe-4x5x130x64-logits40', T=4, E=5, B=130, H=64, big=True),  # gate logits of magnitude 40: saturated
]
MMOE_REFUSED = dict(id='mmoe-refuse-E33', T=1, E=33, B=2, H=8)


def mmoe_inputs(case):
  g = _gen(15)
  T, E, B, H = case['T'], case['E'], case['B'], case['H']
  logits = _randn(g, T, B, E)
  if case.get('big'):
    logits = 40.0 * torch.sign(logits) + _randn(g, T, B, E)
  return dict(experts=_randn(g, E, B, H), logits=logits, dout=_randn(g, T, B, H))


def mmoe_formula(case, inp, dt):
  experts, logits = (_t(inp[k], dt).requires_grad_(True) for k in ('experts', 'logits'))
  gates = torch.softmax(logits, dim=-1)
  out = (gates.permute(0, 2, 1)[..., None] * experts[None]).sum(dim=1)  # softmax (.) experts, summed over experts
  dexperts, dlogits = _grads(out, (experts, logits), _t(inp['dout'], dt))
  return dict(gates=gates, out=out, dexperts=dexperts, dlogits=dlogits)


def mmoe_bound(case, inp):
  T, E, B, H = case['T'], case['E'], case['B'], case['H']
  experts, logits, dout = (_t(inp[k], F64) for k in ('experts', 'logits', 'dout'))
  p, bp = _softmax_bound(logits, torch.zeros_like(logits), E)  # the logits are inputs: no argument error
  xa, ga = experts.abs(), dout.abs()
  b = dict(gates=bp)
  # out[t,b,h] = sum_e p_e x_e: bp_e |x_e| each, a product and E - 1 additions.  n = E, c = 2.
  b['out'] = torch.einsum('tbe,ebh->tbh', bp, xa) + (E + 2) * U * torch.einsum('tbe,ebh->tbh', p, xa)
  # dexperts[e,b,h] = sum_t p[t,b,e] dout[t,b,h].  n = T, c = 2.
  b['dexperts'] = torch.einsum('tbe,tbh->ebh', bp, ga) + (T + 2) * U * torch.einsum('tbe,tbh->ebh', p, ga)
  # dlogits: the softmax gradient over dg_e = sum_h dout_h x_eh (n = H, then n = E for the dot with the gates)
  dg = torch.einsum('tbh,ebh->tbe', dout, experts)
  D = torch.einsum('tbh,ebh->tbe', ga, xa)
  b['dlogits'] = _softmax_grad_bound(p, bp, dg, D, H, E, torch.ones_like(p, dtype=torch.bool), 1.0)
  return b


def run_mmoe(be, case, inp, dev, seen=None):
  experts, logits, dout = (inp[k].to(dev) for k in ('experts', 'logits', 'dout'))
  out, gates = be.mmoe_mix_fwd(experts, logits)
  dexperts, dlogits = be.mmoe_mix_bwd(experts, gates, dout)
  return dict(gates=gates, out=out, dexperts=dexperts, dlogits=dlogits)


# ------------------------------------------------------------------------------------------------------------------
# sigmoid cross-entropy:  loss = loss_scale * sum_i w_i ce(z_i, y_i) / max(#{w_i != 0}, 1),  p = sigmoid(z)
# ------------------------------------------------------------------------------------------------------------------
CE_SPECIAL = (0.0, 1e-4, -1e-4, 20.0, -20.0, 90.0, -90.0)  # naive log(1 + exp(z)) overflows at 90; 1 - p cancels from 20
CE_SCALE = f32(0.7)
CE_CASES = [dict(id='ce-%d-%s' % (B, 'w' if w else 'now'), B=B, weights=w) for B in (1, 300, 4097) for w in (False, True)]


def ce_inputs(case):
  g = _gen(16)
  B = case['B']
  z = 3.0 * _randn(g, B)
  y = (torch.rand(B, generator=g) < 0.5).to(F32)
  w = torch.where(torch.rand(B, generator=g) < 0.5, torch.zeros(B), torch.full((B,), 2.0))
  k = len(CE_SPECIAL)
  if B >= 2 * k:  # every special logit under both labels, with weight 2
    z[:2 * k] = torch.tensor(CE_SPECIAL + CE_SPECIAL)
    y[:k], y[k:2 * k] = 0.0, 1.0
    w[:2 * k] = 2.0
  else:  # one example: the logit whose naive loss overflows, mislabelled
    z[0], y[0], w[0] = 90.0, 0.0, 2.0
  return dict(z=z, y=y, w=w if case['weights'] else None)


def ce_formula(case, inp, dt):
  z, y = _t(inp['z'], dt).requires_grad_(True), _t(inp['y'], dt)
  w = torch.ones_like(z) if inp['w'] is None else _t(inp['w'], dt)
  ce = -(y * torch.nn.functional.logsigmoid(z) + (1 - y) * torch.nn.functional.logsigmoid(-z))
  nz = (w != 0).sum().clamp(min=1).to(dt)
  loss = ((w * ce).sum() / nz * CE_SCALE).reshape(1)
  dz, = _grads(loss, z, torch.ones(1, dtype=dt))
  return dict(loss=loss, dz=dz, p=torch.sigmoid(z))


def ce_bound(case, inp):
  B = case['B']
  z, y = _t(inp['z'], F64), _t(inp['y'], F64)
  w = torch.ones_like(z) if inp['w'] is None else _t(inp['w'], F64)
  nz = float((w != 0).sum().clamp(min=1))
  p = torch.sigmoid(z)
  b = {}
  # p = 1 / (1 + expf(-z)): expf, the addition, the division.  c = EXP_U + 4.  (z = -90: expf overflows, p = 0 against
  # 8e-40: the floor.)
  b['p'] = (EXP_U + 4) * U * p + FLT_MIN
  # dz = loss_scale * w * (p - y) / nz: p's error, the subtraction, three more.  M = loss_scale |w| (p + y) / nz, c = EXP_U + 4 + 8.
  b['dz'] = (EXP_U + 12) * U * CE_SCALE * w.abs() * (p + y) / nz + FLT_MIN
  # loss: ce = max(z, 0) - z y + log1pf(expf(-|z|)) (expf, log1pf, a product, two additions), times w, summed over B,
  # times loss_scale, over nz: six elementwise operations.  n = B, c = EXP_U + LOG_U + 12.
  M = CE_SCALE / nz * (w.abs() * (z.clamp(min=0) + z.abs() * y + torch.log1p(torch.exp(-z.abs())))).sum()
  b['loss'] = ((B + EXP_U + LOG_U + 12) * U * M + FLT_MIN).reshape(1)
  return b


def run_ce(be, case, inp, dev, seen=None):
  w = None if inp['w'] is None else inp['w'].to(dev)
  loss, dz, p = be.sigmoid_ce(inp['z'].to(dev), inp['y'].to(dev), w, CE_SCALE)
  return dict(loss=loss, dz=dz, p=p)


# ------------------------------------------------------------------------------------------------------------------
# CIN (xDeepFM), the four kernels one by one on given float32 operands - no GEMM in between:
#   outer_fwd     z[(b, d), h * H0 + m] = xi[b, h, d] * x0[b, m, d]
#   act_pool_fwd  fm = relu(c + bias) in place,  pooled[b, col0 + n] = sum_d fm[(b, d), n]
#   act_pool_bwd  dc = d(pooled . dpooled + fm . dnext) / dc               (dnext may be absent, dc may BE dnext)
#   outer_bwd     dxi (+)= dz . dz/dxi,  dx0 += dz . dz/dx0
# c and bias are float32, so fl(c + bias) has the sign of the exact sum (it is 0 only when c == -bias, and a sum of two
# floats that is not 0 is at least half an ulp of the larger away from it): the ReLU mask is the same in float32 and
# in float64, and every tensor can be held to a strict bound.
# form 'first': xi IS x0 [B, H0, D] (strides (H0*D, D, 1)), dxi IS dx0 and is added to; form 'later': xi [B, D, H]
# (strides (D*H, 1, H)), dxi its own buffer - written over NaN (add_xi = 0) or added to (add_xi = 1); dx0 is always
# added to.
# ------------------------------------------------------------------------------------------------------------------
CIN_BLOCK = 256           # er::kBlock: columns of z per workgroup, elements per workgroup of the two act_pool kernels
CIN_LDS_BUDGET = 60 * 1024


def cin_outer_bwd_lds(H, H0):
  """er_cin_outer_bwd's LDS bytes: the xi column, the x0 column and one row of dz."""
  return (H + H0 + H * H0) * 4


def _cin_cases():
  cases = []

  def add(form, B, H, H0, D, N, col0, pad, dnext, add_xi):
    cases.append(dict(id='cin-%s-%dx%dx%dx%dx%d-col%dof%d-%s-add%d' % (form, B, H, H0, D, N, col0, col0 + N + pad, dnext, add_xi), form=form,
                      B=B, H=H, H0=H0, D=D, N=N, col0=col0, ld=col0 + N + pad, dnext=dnext, add_xi=add_xi))

  for add_xi in (0, 1):
    add('later', 3, 3, 2, 4, 5, 2, 3, 'present', add_xi)    # K = 6, B*N = 15, B*D*N = 60: everything below one block
    add('later', 2, 16, 16, 3, 7, 0, 0, 'none', add_xi)     # K = 256: exactly one block of z columns; pooled contiguous
    add('later', 2, 17, 16, 2, 3, 1, 2, 'alias', add_xi)    # K = 272: a second block in y, 16 columns of it live
    add('later', 1, 300, 2, 2, 4, 0, 1, 'present', add_xi)  # H > 256: outer_bwd's h loops take two trips
    add('later', 1, 2, 300, 2, 4, 3, 0, 'alias', add_xi)    # H0 > 256: its m loops take two trips
    add('later', 1, 122, 123, 2, 2, 0, 0, 'none', add_xi)   # 61004 bytes of LDS, the largest pair 61440 admits; B*D = 2
    add('later', 5, 3, 2, 3, 65, 4, 2, 'present', add_xi)   # B*N = 325 straddles a block, B*D*N = 975 four of them
    add('later', 7, 4, 1, 3, 1, 1, 1, 'alias', add_xi)      # H0 = 1 (z is xi scaled), N = 1
    add('later', 6, 3, 2, 1, 3, 0, 2, 'present', add_xi)    # D = 1: pooled is fm, a row of z per example
  add('first', 2, 16, 16, 3, 2, 1, 1, 'present', 1)         # the aliased first layer at K = 256
  add('first', 3, 3, 3, 2, 4, 0, 0, 'alias', 1)             # and small
  return cases


CIN_CASES = _cin_cases()
# refused by the host, nothing launched: H = H0 = 123 needs 61500 bytes of LDS; dxi aliasing dx0 without adding;
# H * H0 = 2**24 columns (checked before any access: the buffers are a few floats)
CIN_REFUSED = [dict(id='cin-refuse-lds-123x123', kernel='outer_bwd', form='first', B=1, H=123, H0=123, D=2, add_xi=1,
                    match='too many rows / features'),
               dict(id='cin-refuse-alias-no-add', kernel='outer_bwd', form='first', B=2, H=3, H0=3, D=2, add_xi=0,
                    match='dxi aliasing dx0 must add'),
               dict(id='cin-refuse-K-2pow24', kernel='outer_fwd', form='later', B=1, H=4096, H0=4096, D=1, add_xi=0,
                    match='too many rows / columns')]


def cin_strides(case):
  H, H0, D = case['H'], case['H0'], case['D']
  return (H0 * D, D, 1) if case['form'] == 'first' else (D * H, 1, H)


def cin_inputs(case, seed=17):
  g = _gen(seed)
  B, H, H0, D, N, ld = (case[k] for k in ('B', 'H', 'H0', 'D', 'N', 'ld'))
  inp = dict(x0=_randn(g, B, H0, D), bias=_randn(g, N), c=_randn(g, B * D, N), pooled0=_randn(g, B, ld),
             dpooled=_randn(g, B, ld), dnext=_randn(g, B * D, N), dz=_randn(g, B * D, H * H0), old0=_randn(g, B, H0, D))
  if case['form'] == 'later':
    inp.update(xi=_randn(g, B, D, H), oldi=_randn(g, B, D, H))
  # planted: flat element 0 of c is -bias exactly (fm 0, no gradient), element 1 is one float32 above -bias (fm > 0)
  flat, nb = inp['c'].view(-1), -inp['bias']
  flat[0] = nb[0]
  flat[1] = torch.nextafter(nb[1 % N], torch.tensor(float('inf')))
  inp['fm32'] = torch.relu(inp['c'] + inp['bias'])  # what act_pool_bwd is given: one float32 addition, the same bits anywhere
  return inp


def cin_ties(case):
  """(row, n) of the exact tie and of the entry one ulp above it."""
  N = case['N']
  return (0, 0), (1 // N, 1 % N)


def _cin_outer(xv, x0):
  """xv [B, H, D], x0 [B, H0, D] -> z [(b, d), (h, m)]; all-positive coefficients: its own abs formula on abs inputs."""
  B, H, D = xv.shape
  return (xv.permute(0, 2, 1)[:, :, :, None] * x0.permute(0, 2, 1)[:, :, None, :]).reshape(B * D, H * x0.shape[1])


def _cin_outer_eval(case, inp, dt, absolute):
  c = (lambda k: _t(inp[k], dt).abs()) if absolute else (lambda k: _t(inp[k], dt))
  x0 = c('x0').requires_grad_(True)
  if case['form'] == 'first':  # xi IS x0: both terms of the gradient land in dx0
    z = _cin_outer(x0, x0)
    g0, = _grads(z, (x0,), c('dz'))
    dx0 = c('old0') + g0
    return dict(z=z, dxi=dx0, dx0=dx0)
  xi = c('xi').requires_grad_(True)
  z = _cin_outer(xi.permute(0, 2, 1), x0)
  g0, gi = _grads(z, (x0, xi), c('dz'))
  return dict(z=z, dxi=(c('oldi') + gi) if case['add_xi'] else gi, dx0=c('old0') + g0)


def _cin_act_pool_eval(case, inp, dt, absolute):
  B, D, N, col0 = case['B'], case['D'], case['N'], case['col0']
  sl = slice(col0, col0 + N)
  c = (lambda k: _t(inp[k], dt).abs()) if absolute else (lambda k: _t(inp[k], dt))
  cc, bias = c('c').requires_grad_(True), c('bias')
  if absolute:  # the mask is the true one, a constant; under it fm = c + bias becomes |c| + |bias|
    fm = (_t(inp['c'], dt) + _t(inp['bias'], dt) > 0).to(dt) * (cc + bias)
  else:
    fm = torch.relu(cc + bias)
  pv = fm.reshape(B, D, N).sum(dim=1)
  pooled = c('pooled0').clone()
  pooled[:, sl] = pv
  if case['dnext'] == 'none':
    dc, = _grads(pv, cc, c('dpooled')[:, sl])
  else:
    dc, = _grads((pv, fm), cc, (c('dpooled')[:, sl], c('dnext')))
  return dict(fm=fm, pooled=pooled, dc=dc)


def cin_formula(case, inp, dt):
  r = _cin_outer_eval(case, inp, dt, False)
  r.update(_cin_act_pool_eval(case, inp, dt, False))
  return r


def cin_bound(case, inp):
  H, H0, D, N, col0, add_xi = (case[k] for k in ('H', 'H0', 'D', 'N', 'col0', 'add_xi'))
  M = _cin_outer_eval(case, inp, F64, True)
  M.update(_cin_act_pool_eval(case, inp, F64, True))
  b = {}
  # z: one product.  n = 0, c = 2.
  b['z'] = 2 * U * M['z']
  # fm = relu(c + bias): one addition, the ReLU selects.  n = 0, c = 2; where the mask is off M is 0: fm must BE 0.
  b['fm'] = 2 * U * M['fm']
  # pooled = sum_d fm: fm's addition, then D - 1 more.  n = D, c = 2.  Beside the written columns nothing may move.
  b['pooled'] = torch.zeros_like(M['pooled'])
  b['pooled'][:, col0:col0 + N] = (D + 2) * U * M['pooled'][:, col0:col0 + N]
  # dc = (dpooled + dnext) * mask: one addition, n = 0, c = 2; without dnext a copy of dpooled or a zero: equality
  b['dc'] = torch.zeros_like(M['dc']) if case['dnext'] == 'none' else 2 * U * M['dc']
  if case['form'] == 'first':
    # dx0 = (old + sum_h dz xi) + sum_m dz x0: a monomial of the first sum goes through its product, H - 1 additions and
    # the two accumulations, one of the second through its product, H0 - 1 additions and one accumulation, old through
    # both accumulations.  H == H0 here: n = H, c = 6 (product, accumulate, accumulate) covers all three.
    assert H == H0
    b['dx0'] = b['dxi'] = (H + 6) * U * M['dx0']
  else:
    # dxi = sum_m dz x0: the product, H0 - 1 additions; one more addition, on |old| more, when it adds.
    # n = H0, c = 2 or 4.
    b['dxi'] = (H0 + 2 + 2 * add_xi) * U * M['dxi']
    # dx0 = old + sum_h dz xi: the product, H - 1 additions, the accumulation.  n = H, c = 4.
    b['dx0'] = (H + 4) * U * M['dx0']
  return {k: v.detach() for k, v in b.items()}


def cin_buffers(case, inp, dev):
  """Every operand and destination of the four launches, as the kernels are to find them."""
  B, H, H0, D, N = (case[k] for k in ('B', 'H', 'H0', 'D', 'N'))
  t = lambda k: inp[k].to(dev).clone()
  nan = lambda *shape: torch.full(shape, float('nan'), dtype=F32, device=dev)
  buf = dict(x0=t('x0'), bias=t('bias'), c=t('c'), fm_in=t('fm32'), pooled=t('pooled0'), dpooled=t('dpooled'), dz=t('dz'),
             dx0=t('old0'), z=nan(B * D, H * H0))
  if case['form'] == 'first':
    buf['xi'], buf['dxi'] = buf['x0'], buf['dx0']
  else:
    buf['xi'] = t('xi')
    buf['dxi'] = t('oldi') if case['add_xi'] else nan(B, D, H)  # a write that is skipped leaves a NaN
  buf['dnext'] = None if case['dnext'] == 'none' else t('dnext')
  buf['dc'] = buf['dnext'] if case['dnext'] == 'alias' else nan(B * D, N)
  return buf


def cin_launch(be, case, buf):
  B, H, D, col0 = case['B'], case['H'], case['D'], case['col0']
  strides = cin_strides(case)
  be.cin_outer_fwd(buf['xi'], strides, H, buf['x0'], buf['z'])
  be.cin_act_pool_fwd(buf['c'], buf['bias'], B, D, buf['pooled'], col0)
  be.cin_act_pool_bwd(buf['fm_in'], buf['dpooled'], col0, buf['dnext'], B, D, buf['dc'])
  be.cin_outer_bwd(buf['dz'], buf['xi'], strides, H, buf['x0'], buf['dxi'], bool(case['add_xi']), buf['dx0'])


def cin_results(buf):
  return dict(z=buf['z'], fm=buf['c'], pooled=buf['pooled'], dc=buf['dc'], dxi=buf['dxi'], dx0=buf['dx0'])


def run_cin(be, case, inp, dev, seen=None):
  buf = cin_buffers(case, inp, dev)
  cin_launch(be, case, buf)
  return cin_results(buf)


# ------------------------------------------------------------------------------------------------------------------
# DLRM dot interaction:  out[b, p] = e_i . e_j over the pairs p = (i, j), i ascending, j from i (self_interaction) or
# i + 1 ascending
# ------------------------------------------------------------------------------------------------------------------
# layouts: 'contig' = the backend's defaults (its own out and dx; accumulate into a contiguous buffer);
# 'wide' = x, out, g and dx are each columns [DOT_OFF, DOT_OFF + width) of a wider buffer whose row stride is no
# multiple of 4 floats: the base is 4 bytes off a 16-byte boundary, every row starts at another alignment, and the
# columns beside the operand hold values that must come back bit for bit
DOT_OFF = 1
DOT_LDS_BUDGET = 60 * 1024
DOT_SHAPES = [(5, 2, 3), (3, 9, 1), (4, 27, 16), (1, 40, 8)]
# (5, 2, 3): the minimum F, one pair; (3, 9, 1): D = 1; (4, 27, 16): P = 351 and F*D = 432, both loops past one block;
# (1, 40, 8): one example, P = 780 / 820 four trips


def dot_pairs(F, si):
  return F * (F - 1) // 2 + (F if si else 0)


def dot_fwd_lds(F, D):
  return 4 * F * (D + 1)


def dot_bwd_lds(F, D, si):
  return 4 * (F * (D + 1) + dot_pairs(F, si))


def _dot_cases():
  cases = [dict(id='dot-%dx%dx%d-si%d-%s' % (B, F, D, si, lay), B=B, F=F, D=D, si=bool(si), layout=lay, fwd_only=False)
           for B, F, D in DOT_SHAPES for si in (0, 1) for lay in ('contig', 'wide')]
  # 33280 bytes of LDS forward, 65792 backward: the forward runs, the backward is refused (DOT_REFUSED)
  cases.append(dict(id='dot-1x128x64-si0-contig-fwdonly', B=1, F=128, D=64, si=False, layout='contig', fwd_only=True))
  return cases


DOT_CASES = _dot_cases()
# refused by the host, nothing launched.  what: the ER_REQUIRE that must fire
DOT_REFUSED = [dict(id='dot-refuse-fwd-lds', what='fwd_lds', B=1, F=128, D=120, si=False, match='exceed the LDS budget'),
               dict(id='dot-refuse-bwd-lds', what='bwd_lds', B=1, F=128, D=64, si=False, match='exceed the LDS budget'),
               dict(id='dot-refuse-out-stride', what='out_stride', B=2, F=4, D=3, si=True, match='out_stride'),
               dict(id='dot-refuse-g-stride', what='g_stride', B=2, F=4, D=3, si=True, match='g_stride')]


def dot_ld(case, width):
  """Row stride of the buffer an operand of `width` columns sits in."""
  if case['layout'] == 'contig':
    return width
  ld = width + DOT_OFF + 2
  return ld + 1 if ld % 4 == 0 else ld


def dot_view(buf, case, width):
  return buf if case['layout'] == 'contig' else buf[:, DOT_OFF:DOT_OFF + width]


def dot_inputs(case):
  g = _gen(18)
  B, n, P = case['B'], case['F'] * case['D'], dot_pairs(case['F'], case['si'])
  return dict(xw=_randn(g, B, dot_ld(case, n)), gw=_randn(g, B, dot_ld(case, P)), out0=_randn(g, B, dot_ld(case, P)),
              old=_randn(g, B, dot_ld(case, n)))


def _dot(e, si):  # all-positive coefficients: its own abs formula on abs inputs
  F = e.shape[1]
  i, j = torch.triu_indices(F, F, 0 if si else 1)  # row by row: i ascending, then j
  return torch.einsum('bnd,bmd->bnm', e, e)[:, i, j]


def _dot_eval(case, inp, dt, absolute):
  B, F, D = case['B'], case['F'], case['D']
  n, P = F * D, dot_pairs(F, case['si'])
  c = (lambda k: _t(inp[k], dt).abs()) if absolute else (lambda k: _t(inp[k], dt))
  x = dot_view(c('xw'), case, n).contiguous().requires_grad_(True)
  o = _dot(x.reshape(B, F, D), case['si'])
  out = c('out0').clone()
  dot_view(out, case, P).copy_(o)
  if case['fwd_only']:
    return dict(out=out.detach())
  g, = _grads(o, x, dot_view(c('gw'), case, P))
  dx, acc = c('old').clone(), c('old').clone()
  dot_view(dx, case, n).copy_(g)
  dot_view(acc, case, n).add_(g)
  return dict(out=out.detach(), dx=dx, dx_acc=acc)


def dot_formula(case, inp, dt):
  return _dot_eval(case, inp, dt, False)


def dot_bound(case, inp):
  F, D = case['F'], case['D']
  n, P = F * D, dot_pairs(F, case['si'])
  M = _dot_eval(case, inp, F64, True)

  def inside(key, width, factor):  # beside the operand's columns nothing may move
    b = torch.zeros_like(M[key])
    dot_view(b, case, width).copy_(factor * U * dot_view(M[key], case, width))
    return b

  # out = sum_d e_i e_j: the product, D - 1 additions.  n = D, c = 2.
  b = dict(out=inside('out', P, D + 2))
  if not case['fwd_only']:
    # dx_f = sum over the partners o of g_(f, o) e_o: at most F terms (the self term is 2 g e, the doubling exact), a
    # product each.  n = F, c = 2; accumulating is one more addition, on |old| more: c = 4.
    b['dx'] = inside('dx', n, F + 2)
    b['dx_acc'] = inside('dx_acc', n, F + 4)
  return b


def run_dot(be, case, inp, dev, seen=None):
  F, D, si = case['F'], case['D'], case['si']
  n, P = F * D, dot_pairs(F, si)
  wide = case['layout'] == 'wide'
  x = dot_view(inp['xw'].to(dev), case, n)
  out = inp['out0'].to(dev).clone()
  if wide:
    be.dot_interaction_fwd(x, F, D, si, out=dot_view(out, case, P))
  else:
    out = be.dot_interaction_fwd(x, F, D, si)
  if case['fwd_only']:
    return dict(out=out)
  g = dot_view(inp['gw'].to(dev), case, P)
  dx, acc = inp['old'].to(dev).clone(), inp['old'].to(dev).clone()
  if wide:  # accumulate = 0 into NaN: an element that is not written, or is added to, stays NaN
    dot_view(dx, case, n).fill_(float('nan'))
    be.dot_interaction_bwd(x, g, F, D, si, into=dot_view(dx, case, n), accumulate=False)
  else:
    dx = be.dot_interaction_bwd(x, g, F, D, si)
  be.dot_interaction_bwd(x, g, F, D, si, into=dot_view(acc, case, n), accumulate=True)
  if seen is not None:  # addresses and row strides of the four strided operands
    views = (x, dot_view(out, case, P), g, dot_view(acc, case, n))
    seen.update(ptrs=[v.data_ptr() for v in views], strides=[v.stride(0) for v in views])
  return dict(out=out, dx=dx, dx_acc=acc)


# ------------------------------------------------------------------------------------------------------------------
# the registry: per operation its cases, inputs, formula, bound and runner; references are computed once and shared
# ------------------------------------------------------------------------------------------------------------------
OPS = {
    'fm': (FM_CASES, fm_inputs, fm_formula, fm_bound, run_fm),
    'cross_v1': (CROSS_V1_CASES, cross_v1_inputs, cross_v1_formula, cross_v1_bound, run_cross_v1),
    'din': (DIN_CASES, din_inputs, din_formula, din_bound, run_din),
    'mmoe': (MMOE_CASES, mmoe_inputs, mmoe_formula, mmoe_bound, run_mmoe),
    'ce': (CE_CASES, ce_inputs, ce_formula, ce_bound, run_ce),
    'cin': (CIN_CASES, cin_inputs, cin_formula, cin_bound, run_cin),
    'dot': (DOT_CASES, dot_inputs, dot_formula, dot_bound, run_dot),
}
ALL_CASES = [(op, c) for op in OPS for c in OPS[op][0]]


def case_by_id(op, cid):
  return next(c for c in (CROSS_V2_CASES if op == 'cross_v2' else OPS[op][0]) if c['id'] == cid)


def _frozen(d):
  return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def reference(op, cid):
  """(inputs, fp64 reference, bound) of a case; computed once, shared, never written to."""
  case = case_by_id(op, cid)
  _, inputs, formula, bound, _ = OPS[op]
  inp = inputs(case)
  return inp, _frozen(formula(case, inp, F64)), _frozen(bound(case, inp))


def plain_f32(op, cid):
  case = case_by_id(op, cid)
  return OPS[op][2](case, reference(op, cid)[0], F32)


def run(op, be, cid, dev='cpu', seen=None):
  case = case_by_id(op, cid)
  return OPS[op][4](be, case, reference(op, cid)[0], dev, seen)


@functools.lru_cache(maxsize=None)
def cross_v2_inputs_of(cid):
  return cross_v2_inputs(case_by_id('cross_v2', cid))


@functools.lru_cache(maxsize=None)
def cross_v2_reference(cid, variant):
  case, inp = case_by_id('cross_v2', cid), cross_v2_inputs_of(cid)
  return cross_v2_formula(case, inp, F64, variant), cross_v2_bound(case, inp, variant)


@functools.lru_cache(maxsize=None)
def cross_v2_plain_reference(cid, diag, has_bias):
  case, inp = case_by_id('cross_v2', cid), cross_v2_inputs_of(cid)
  return _frozen(cross_v2_plain_formula(case, inp, F64, diag, has_bias)), _frozen(cross_v2_plain_bound(case, inp, diag, has_bias))
