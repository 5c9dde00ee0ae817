"""The split-weight MFMA NoisyLinear kernels
(machin_amd/ops/hip/noisy_linear_mfma.hip) against float64 references.

Every test calls ``ops._NoisyLinearMFMA`` itself, so none depends on the
value of ``ops.NOISY_LINEAR_MFMA_MIN_BATCH``. ``x`` and ``dy`` are bf16.
"""
from types import SimpleNamespace

import pytest
import torch as t

pytestmark = pytest.mark.gpu

if not t.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from machin_amd import ops  # noqa: E402
from machin_amd.model.nets import ImplicitQuantileHead  # noqa: E402
from util_noisy_linear import (  # noqa: E402
    inputs, make_case, reference64, run, worst_ratio,
)

DEV = "cuda:0"
BF16 = t.bfloat16
OUTPUTS = ("y", "dx", "dmu", "dsigma", "dbias_mu", "dbias_sigma")
# (rows, I, O). Tiles are 64 x 64 with reduction steps of 64; the loaders
# branch on the row length of the a operand (16-byte loads when it is a
# multiple of 8) and, forward, of mu / sigma (float4 when I % 4 == 0):
#   (1,1,1) .. (64,257,130)  scalar loads everywhere, 1 to 5 steps
#   (129,520,70) (300,512,306) (130,3136,6)  forward 16-byte x and float4
#       weights, dx scalar dy; 3 and 5 row steps in the weight gradient
#   (70,36,136)  I % 8 == 4: forward float4 weights whose second group
#       is past the edge, scalar x; O % 8 == 0: dx with 16-byte dy loads
#       over 3 steps, the last one 8 wide
SHAPES = [(1, 1, 1), (33, 65, 17), (64, 257, 130), (129, 520, 70),
          (300, 512, 306), (130, 3136, 6), (70, 36, 136)]
ALL = pytest.mark.parametrize("shape", SHAPES,
                              ids=["x".join(map(str, s)) for s in SHAPES])


def kernel(*args):
    return ops._NoisyLinearMFMA.apply(*args)


def assert_same_bits(got, want, names=OUTPUTS):
    for name in names:
        g, w = getattr(got, name), getattr(want, name)
        assert g.shape == w.shape and g.dtype == w.dtype, name
        assert t.equal(g.cpu().double(), w.cpu().double()), name


@ALL
def test_exact_on_integers(shape):
    """Integers: every product and partial sum is exact, ``lo`` is zero;
    all six outputs equal the float64 reference bit for bit."""
    ref, _ = reference64(shape, "int", BF16)
    got = run(kernel, make_case(shape, "int"), BF16, DEV)
    want = SimpleNamespace(**{
        n: getattr(ref, n).to(BF16 if n in ("y", "dx") else t.float32)
        for n in OUTPUTS})
    assert_same_bits(got, want)


@ALL
def test_exact_on_a_grid_of_2_to_the_minus_8(shape):
    """``mu`` on a 2^-8 grid: ``w`` has at most 16 significant bits, so
    ``hi + lo == w`` and every partial sum is a multiple of 2^-8 below
    2^16: y and dx equal the bf16-rounded float64 reference bit for bit.
    A kernel that drops ``lo`` fails here."""
    B, I, O = shape
    base = make_case(shape, "int")
    gen = t.Generator().manual_seed(B + 7 * I + 49 * O)
    case = SimpleNamespace(**vars(base))
    case.weight_mu = base.weight_mu \
        + t.randint(0, 256, (O, I), generator=gen).float() / 256
    x, dy = (v.double() for v in inputs(case, BF16))
    outer = t.outer(case.eps_out, case.eps_in).double()
    w = case.weight_mu.double() + case.weight_sigma.double() * outer
    want = SimpleNamespace(
        y=(x @ w.t() + case.bias_mu.double()
           + case.bias_sigma.double() * case.eps_out.double()).to(BF16),
        dx=(dy @ w).to(BF16))
    assert_same_bits(run(kernel, case, BF16, DEV), want, ("y", "dx"))


@ALL
def test_rounding_bound(shape):
    """The util's fp32 bound as it is for the parameter gradients; for y
    and dx plus ``2^-16 S`` for the 16-bit weight:
    ``(K + 8 + 256) 2^-24 S + 2^-8 |ref|``."""
    B, I, O = shape
    ref, bound = reference64(shape, "randn", BF16)
    bound = SimpleNamespace(**vars(bound))
    for name, k in (("y", I), ("dx", O)):
        store = 2.0 ** -8 * getattr(ref, name).abs()
        acc = getattr(bound, name) - store  # (k + 8) 2^-24 S
        setattr(bound, name, acc * (k + 8 + 256) / (k + 8) + store)
    got = run(kernel, make_case(shape, "randn"), BF16, DEV)
    ratio, where = worst_ratio(got, ref, bound)
    print(f"{shape}: worst |err| / bound = {ratio:.3f} ({where})")
    assert ratio <= 1.0, where


@pytest.mark.parametrize("shape", [(300, 512, 306), (130, 3136, 6)],
                         ids=["300x512x306", "130x3136x6"])
def test_deterministic_and_without_input_gradient(shape):
    case = make_case(shape, "randn")
    one = run(kernel, case, BF16, DEV)
    assert_same_bits(run(kernel, case, BF16, DEV), one)
    part = run(kernel, case, BF16, DEV, x_grad=False)
    assert part.dx is None
    assert_same_bits(part, one, [n for n in OUTPUTS if n != "dx"])


def test_dispatch(monkeypatch):
    """bf16 x from the limit on takes the MFMA kernels; fewer rows, and
    fp32 x of any row count, keep the torch form, bit for bit."""
    monkeypatch.setattr(ops, "NOISY_LINEAR_MFMA_MIN_BATCH", 64)
    used = []
    real = ops._NoisyLinearMFMA.apply
    monkeypatch.setattr(ops._NoisyLinearMFMA, "apply",
                        lambda *a: used.append(1) or real(*a))
    for rows, dtype, mfma in ((64, BF16, True), (63, BF16, False),
                              (64, t.float32, False)):
        case = make_case((rows, 65, 17), "randn")
        used.clear()
        got = run(ops.noisy_linear, case, dtype, DEV)
        assert bool(used) == mfma
        want = run(real if mfma else ops._noisy_linear_torch, case, dtype,
                   DEV)
        assert_same_bits(got, want)


def test_implicit_quantile_head(monkeypatch):
    """A noisy IQN head of 128 rows on the MFMA path against the same head
    on the torch form. Each layer is off its exact value by at most
    ``(K + 8 [+ 256]) 2^-24 S + 2^-8 |value|`` on either path (``S`` the
    sum of its absolute terms), so the two differ by the sum of both; as
    in ``head_bound`` a layer's input error is multiplied by ``|w|``. In
    the backward a hidden unit within its error of zero may pass on one
    path and not on the other, which adds its whole gradient; the
    embedding's backward sums 32 products ``dh * phi`` in fp32 on both
    paths and stores bf16."""
    t.manual_seed(5)
    head = ImplicitQuantileHead(64, 3, hidden=40, n_cos=16, noisy=True)
    head = head.to(DEV)
    feature = t.randn(4, 64, device=DEV).to(BF16).requires_grad_(True)
    taus = t.rand(4, 32, device=DEV)
    dq = t.randn(4, 3, 32, device=DEV)

    def once(limit):
        monkeypatch.setattr(ops, "NOISY_LINEAR_MFMA_MIN_BATCH", limit)
        kept = {}
        hook = head.embedding.register_forward_hook(
            lambda m, i, o: kept.update(h=o))
        q = head(feature, taus)
        grad, = t.autograd.grad(q, feature, dq)
        hook.remove()
        return q.detach(), grad, kept["h"].detach()

    q_a, g_a, h = once(64)
    q_b, g_b, _ = once(129)
    assert bool(t.isfinite(q_a).all()) and bool(t.isfinite(g_a).all())

    u, store = 2.0 ** -24, 2.0 ** -8
    h = h.double().view(128, 64)

    def exact(layer):
        p = [v.detach().double() for v in (
            layer.weight_mu, layer.weight_sigma, layer.bias_mu,
            layer.bias_sigma, layer.eps_in, layer.eps_out)]
        outer = t.outer(p[5], p[4])
        return (p[0] + p[1] * outer, p[2] + p[3] * p[5],
                p[0].abs() + (p[1] * outer).abs())

    def layer_err(x, x_err, w, b, w_abs):
        # both paths together: (K + 8) + (K + 8 + 256), two bf16 stores
        y = x @ w.t() + b
        s = x.abs() @ w_abs.t() + b.abs()
        k = 2 * (w.shape[1] + 8) + 256
        return y, (x_err @ w_abs.t() + k * u * s) * (1 + store) \
            + 2 * store * y.abs()

    w1, b1, a1 = exact(head.hidden)
    w2, b2, a2 = exact(head.out)
    y1, e1 = layer_err(h, t.zeros_like(h), w1, b1, a1)
    _, e2 = layer_err(t.relu(y1), e1, w2, b2, a2)
    e_q = e2.view(4, 32, 3).transpose(1, 2)
    assert bool(((q_a - q_b).abs().double() <= e_q).all())

    # backward: dq -> bf16 -> out layer dx -> ReLU mask -> hidden layer dx
    g = dq.transpose(1, 2).reshape(128, 3).to(BF16).double()
    zero = t.zeros(1, dtype=t.float64, device=DEV)
    d2, e_d2 = layer_err(g, t.zeros_like(g), w2.t(), zero, a2.t())
    flip = (y1.abs() <= e1).double()
    e_dr = t.where(y1 > -e1, e_d2, t.zeros_like(e_d2)) \
        + flip * (d2.abs() + e_d2)
    d1, e_d1 = layer_err(d2 * (y1 > 0), e_dr, w1.t(), zero, a1.t())
    # embedding backward: dfeature[b] = sum_n dh[b, n] phi[b, n], phi >= 0
    emb = head.embedding
    # (the kernel's fp32 phi is the same on both paths and within 2^-8
    # of the exact one by a wide margin)
    i = t.arange(16, device=DEV, dtype=t.float64)
    cos = t.cos(t.pi * i * taus.double().unsqueeze(-1))
    phi = t.relu(cos @ emb.weight.detach().double().t()
                 + emb.bias.detach().double()) * (1 + store)
    d_abs = (d1.abs() + e_d1).view(4, 32, 64)
    e_g = (e_d1.view(4, 32, 64) * phi).sum(1) \
        + 2 * (32 + 8) * u * (d_abs * phi).sum(1) \
        + store * (g_a.abs() + g_b.abs()).double()
    assert bool(((g_a - g_b).abs().double() <= e_g).all())
