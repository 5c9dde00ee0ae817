"""Shared inputs, float64 references and error bounds for the
``ops.noisy_linear`` tests.

Everything returned from the cached functions here is shared between
tests: do not modify it in place.
"""
import functools
from types import SimpleNamespace

import torch as t

# (B, I, O). Small and odd edges; several batch tiles with the 6 x 51
# head; the real first layer. The kernels' tiles are 32 (batch) x 64
# (outputs) x 64 (reduction) forward and for dx, 32 (O) x 64 (I) x 32
# (batch) for the weight gradient: (7,64,64), (33,65,17), (64,257,130),
# (65,128,3) and (31,63,33) sit on, one above and one below those edges.
#
# The forward and dx also cut their reduction into S slices of `cps`
# 64-element steps so that about 512 blocks run (SLICES below repeats
# the policy). Up to (32,3136,512) every shape has cps == 1, so a block
# runs one step; the last four make blocks loop over several steps,
# with S > 1 and with S == 1 (direct store with bias and bf16 rounding),
# with float4 (I % 4 == 0) and scalar weight loads, and with a last
# slice that is shorter than the others:
#   (2100,520,70)   forward S=3 cps=3;            dx S=1, 2 steps
#   (1000,777,100)  forward S=7 cps=2, last 1;    dx S=2 cps=1
#   (530,130,2048)  forward S=1, 3 steps;         dx S=11 cps=3, last 2
#   (530,132,2048)  the same with float4 loads
SHAPES = [
    (1, 1, 1), (2, 3, 5), (7, 64, 64), (33, 65, 17), (64, 257, 130),
    (65, 128, 3), (31, 63, 33), (300, 512, 306), (32, 3136, 512),
    (2100, 520, 70), (1000, 777, 100), (530, 130, 2048), (530, 132, 2048),
]
MULTI_STEP_SHAPES = SHAPES[-4:]
BIG_SHAPES = [(300, 512, 306), (32, 3136, 512)] + MULTI_STEP_SHAPES
# (S, cps) of the forward and of dx, as listed above
SLICES = {
    (2100, 520, 70): ((3, 3), (1, 2)),
    (1000, 777, 100): ((7, 2), (2, 1)),
    (530, 130, 2048): ((1, 3), (11, 3)),
    (530, 132, 2048): ((1, 3), (11, 3)),
}
OUTPUTS = ("y", "dx", "dmu", "dsigma", "dbias_mu", "dbias_sigma")
PARAMS = ("weight_mu", "weight_sigma", "bias_mu", "bias_sigma")


def shape_id(shape):
    return "x".join(str(s) for s in shape)


SHAPE_IDS = [shape_id(s) for s in SHAPES]


def f_noise(z):
    return z.sign() * z.abs().sqrt()


@functools.lru_cache(maxsize=None)
def make_case(shape, kind):
    """fp32 inputs on the CPU. ``kind='int'``: small integers, so that
    every product and partial sum is an integer below 2^24 and fp32
    accumulation is exact in any order. ``kind='randn'``: normal x and
    dy, parameters at their init scale, noise ``f(randn)``."""
    B, I, O = shape
    gen = t.Generator().manual_seed(B * 1000003 + I * 1009 + O)

    def ints(lo, hi, *size):
        return t.randint(lo, hi + 1, size, generator=gen).float()

    if kind == "int":
        return SimpleNamespace(
            shape=shape, x=ints(-2, 2, B, I), dy=ints(-2, 2, B, O),
            weight_mu=ints(-3, 3, O, I), weight_sigma=ints(0, 2, O, I),
            bias_mu=ints(-3, 3, O), bias_sigma=ints(0, 2, O),
            eps_in=ints(-2, 2, I), eps_out=ints(-2, 2, O),
        )
    assert kind == "randn"
    bound = 1.0 / I ** 0.5
    return SimpleNamespace(
        shape=shape,
        x=t.randn(B, I, generator=gen), dy=t.randn(B, O, generator=gen),
        weight_mu=(t.rand(O, I, generator=gen) * 2 - 1) * bound,
        weight_sigma=t.full((O, I), 0.5 * bound),
        bias_mu=(t.rand(O, generator=gen) * 2 - 1) * bound,
        bias_sigma=t.full((O,), 0.5 * bound),
        eps_in=f_noise(t.randn(I, generator=gen)),
        eps_out=f_noise(t.randn(O, generator=gen)),
    )


def inputs(case, dtype):
    """``(x, dy)`` as the op sees them in ``dtype`` (bf16: rounded)."""
    return case.x.to(dtype), case.dy.to(dtype)


@functools.lru_cache(maxsize=None)
def reference64(shape, kind, dtype):
    """The six outputs from the formulas in float64 (composed weight),
    with x and dy first rounded to ``dtype``, and the worst-case
    rounding bound of each for fp32 accumulation in any order:
    ``(K + 8) * 2^-24 * S`` with ``S`` the sum of the absolute values of
    the output's terms and ``K`` its reduction length, plus
    ``2^-8 |ref|`` where the output is stored in bf16."""
    case = make_case(shape, kind)
    B, I, O = shape
    x, dy = (v.double() for v in inputs(case, dtype))
    mu, sigma = case.weight_mu.double(), case.weight_sigma.double()
    bmu, bsig = case.bias_mu.double(), case.bias_sigma.double()
    ei, eo = case.eps_in.double(), case.eps_out.double()
    outer = eo.view(O, 1) * ei.view(1, I)
    w = mu + sigma * outer
    ref = SimpleNamespace(
        y=x @ w.t() + bmu + bsig * eo,
        dx=dy @ w,
        dmu=dy.t() @ x,
        dbias_mu=dy.sum(dim=0),
    )
    ref.dsigma = ref.dmu * outer
    ref.dbias_sigma = ref.dbias_mu * eo
    w_abs = mu.abs() + (sigma * outer).abs()
    s_dmu = dy.abs().t() @ x.abs()
    s_dbias = dy.abs().sum(dim=0)
    sums = dict(
        y=(x.abs() @ w_abs.t() + bmu.abs() + (bsig * eo).abs(), I),
        dx=(dy.abs() @ w_abs, O),
        dmu=(s_dmu, B),
        dsigma=(s_dmu * outer.abs(), B),
        dbias_mu=(s_dbias, B),
        dbias_sigma=(s_dbias * eo.abs(), B),
    )
    bound = SimpleNamespace()
    for name, (s, k) in sums.items():
        b = (k + 8) * 2.0 ** -24 * s
        if dtype == t.bfloat16 and name in ("y", "dx"):
            b = b + 2.0 ** -8 * getattr(ref, name).abs()
        setattr(bound, name, b)
    return ref, bound


def run(fn, case, dtype, device="cpu", x_grad=True, param_dtype=None):
    """Forward and backward of ``fn(x, mu, sigma, bias_mu, bias_sigma,
    eps_in, eps_out)`` on a case: a namespace of the six outputs
    (``dx`` is None without ``x_grad``), detached, on ``device``."""
    x, dy = (v.to(device) for v in inputs(case, dtype))
    if param_dtype is not None:
        x, dy = x.to(param_dtype), dy.to(param_dtype)
    x = x.clone().requires_grad_(x_grad)
    params = [
        getattr(case, n).to(device=device, dtype=param_dtype or t.float32)
        .clone().requires_grad_(True) for n in PARAMS
    ]
    eps = [getattr(case, n).to(device=device, dtype=param_dtype or t.float32)
           for n in ("eps_in", "eps_out")]
    y = fn(x, *params, *eps)
    y.backward(dy)
    return SimpleNamespace(
        y=y.detach(), dx=x.grad, dmu=params[0].grad, dsigma=params[1].grad,
        dbias_mu=params[2].grad, dbias_sigma=params[3].grad,
    )


def worst_ratio(got, ref, bound, names=OUTPUTS):
    """Largest ``|got - ref| / bound`` over the named outputs (elements
    whose bound is zero must match exactly), with the output's name."""
    worst, where = 0.0, None
    for name in names:
        g = getattr(got, name).detach().cpu().double()
        r, b = getattr(ref, name), getattr(bound, name)
        assert g.shape == r.shape, name
        assert bool(t.isfinite(g).all()), name
        err = (g - r).abs()
        zero = b == 0
        assert bool((err[zero] == 0).all()), name
        ratio = float((err[~zero] / b[~zero]).max()) if (~zero).any() else 0.0
        if ratio > worst:
            worst, where = ratio, name
    return worst, where


def head_bound(exact, feat, dtype):
    """Worst-case error of ``NoisyDuelingC51Head`` computed in fp32 with
    layer outputs stored in ``dtype``, per logit, from the float64 head
    ``exact`` and its float64 input. A layer's fp32 output is off by at
    most ``(I + 8) 2^-24 S`` (S the sum of its absolute terms) and a
    bf16 store adds ``2^-8`` of the stored value; the hidden layer's
    error passes the 1-Lipschitz ReLU and is multiplied by ``|w|`` of
    the output layer; the aggregation ``v + a - mean(a)`` passes the
    errors on and adds three fp32 roundings of values no larger than
    ``|v| + 2 max|a|``."""
    store = 2.0 ** -8 if dtype == t.bfloat16 else 0.0

    def w_abs(layer):
        outer = t.outer(layer.eps_out, layer.eps_in)
        return (layer.weight_mu.abs()
                + (layer.weight_sigma * outer).abs()).detach()

    def layer_bound(layer, x, x_err):
        y = layer(x).detach()
        s = x.abs() @ w_abs(layer).t() + layer.bias_mu.abs() \
            + (layer.bias_sigma * layer.eps_out).abs()
        err = x_err @ w_abs(layer).t() \
            + (layer.in_features + 8) * 2.0 ** -24 * s.detach()
        return y, err * (1 + store) + store * y.abs()

    def stream(hidden, out):
        h, e_h = layer_bound(hidden, feat, t.zeros_like(feat))
        return layer_bound(out, t.relu(h), e_h)

    v, e_v = stream(exact.value_hidden, exact.value_out)
    a, e_a = stream(exact.advantage_hidden, exact.advantage_out)
    rows, atoms = v.shape
    v, e_v = v.view(rows, 1, atoms), e_v.view(rows, 1, atoms)
    a, e_a = a.view(rows, -1, atoms), e_a.view(rows, -1, atoms)
    size = v.abs() + 2 * a.abs().amax(dim=1, keepdim=True)
    return e_v + e_a + e_a.mean(dim=1, keepdim=True) \
        + 3 * 2.0 ** -24 * size
