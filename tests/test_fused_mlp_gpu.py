"""GPU tests of the fused MLP kernels (machin_amd/ops/hip/fused_mlp.hip)
against a float64 reference: exactly on sparse integer inputs, and on
general inputs within 4 times the error of the fp32 torch form on the
device plus 2^-22 (both are fp32 sums of the same terms in other orders).

MEASURED on one MI355X, worst kernel error / torch-form error over the
outputs of a case (both relative to the float64 tensor's largest value),
and the largest kernel error: (1, 1, 1) 1.00, 2.0e-7; (5, 130, 64, 3)
1.38, 2.9e-7; E = 2 (17, 256, 256, 6) 1.11, 3.0e-7; E = 3 (3, 16, 1)
1.00, 6.9e-8; (24, 200, 40, 72, 2) 1.43, 3.1e-7; (8, 64, 64, 4) 1.43,
1.8e-7. The bound is 4 plus the floor.
"""
import functools

import pytest
import torch as t

pytestmark = pytest.mark.gpu

if not t.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from machin_amd import ops  # noqa: E402
from machin_amd.model.nets import FusedMLP  # noqa: E402

DEV = "cuda:0"
# (E, B, sizes, shared x)
CASES = [
    (None, 1, (1, 1, 1), False),
    (None, 33, (5, 130, 64, 3), False),
    (2, 70, (17, 256, 256, 6), True),
    (3, 5, (3, 16, 1), False),
    (None, 40, (24, 200, 40, 72, 2), False),
    (None, 261, (8, 64, 64, 4), False),
]
cases = pytest.mark.parametrize("case", range(len(CASES)),
                                ids=[str(c) for c in CASES])


def reference(x, ws, bs, dy, absolute=False):
    """float64, ensemble form (x [E or 1, B, K]). Returns the outputs
    [y, dx, dW.., db..], the hidden pre-activations and their sums of
    absolute terms. ``absolute``: no mask, for the network of absolute
    values."""
    a, zs, sums = [x], [], []
    for l, (w, b) in enumerate(zip(ws, bs)):
        z = a[-1] @ w.transpose(1, 2) + b[:, None]
        if l < len(ws) - 1:
            zs.append(z)
            sums.append(a[-1].abs() @ w.abs().transpose(1, 2)
                        + b.abs()[:, None])
        a.append(z.clamp_min(0) if l < len(ws) - 1 else z)
    g, dws, dbs = dy, [], []
    for l in reversed(range(len(ws))):
        if l < len(ws) - 1 and not absolute:
            g = g * (zs[l] > 0)
        dws.insert(0, g.transpose(1, 2) @ a[l].expand(len(g), -1, -1))
        dbs.insert(0, g.sum(1))
        g = g @ ws[l]
    dx = g.sum(0, keepdim=True) if x.shape[0] != g.shape[0] else g
    return [a[-1], dx] + dws + dbs, zs, sums


def run(fn, case, x, ws, bs, dy, need_x=True):
    """fn on the device in fp32, from ensemble-form float64 CPU tensors;
    the outputs come back like the reference's."""
    E, _, _, shared = CASES[case]
    dev = [v.float().to(DEV) for v in [x, dy] + ws + bs]
    if E is None or shared:
        dev[0] = dev[0][0]
    if E is None:
        dev[1:] = [v[0] for v in dev[1:]]
    xd, dyd, params = dev[0].requires_grad_(need_x), dev[1], dev[2:]
    for p in params:
        p.requires_grad_(True)
    y = fn(xd, params[:len(ws)], params[len(ws):])
    y.backward(dyd)
    out = [y.detach(), xd.grad] + [p.grad for p in params]
    full = [None if v is None else
            (v[None] if E is None or (i == 1 and shared) else v)
            for i, v in enumerate(out)]
    return full


@functools.lru_cache(maxsize=None)
def exact_inputs(case):
    E, B, sizes, shared = CASES[case]
    gen = t.Generator().manual_seed(100 + case)
    density = 0.125 if max(sizes) >= 64 else 0.5

    def sparse(*shape):
        v = t.randint(-1, 2, shape, generator=gen).double()
        return v * (t.rand(shape, generator=gen) < density)

    n = E or 1
    x = sparse(1 if shared else n, B, sizes[0])
    ws = [sparse(n, sizes[l + 1], sizes[l]) for l in range(len(sizes) - 1)]
    bs = [sparse(n, sizes[l + 1]) for l in range(len(sizes) - 1)]
    dy = sparse(n, B, sizes[-1])
    x[:, 0], bs[0][:, 0] = 0.0, 0.0   # a pre-activation of exactly 0
    return x, ws, bs, dy


@functools.lru_cache(maxsize=None)
def general_inputs(case):
    E, B, sizes, shared = CASES[case]
    # seeds checked on the float64 reference alone: no ambiguous row in
    # any case (other seeds give up to 6 % in the 256-wide case)
    t.manual_seed(250 + case)
    net = FusedMLP(sizes, ensemble=E or 1)
    ws = [w.detach().double() for w in net.weights]
    bs = [b.detach().double() for b in net.biases]
    gen = t.Generator().manual_seed(300 + case)
    x = t.randn(1 if shared else E or 1, B, sizes[0], generator=gen).double()
    dy = t.randn(E or 1, B, sizes[-1], generator=gen).double()
    _, zs, sums = reference(x, ws, bs, dy)
    ambiguous = t.zeros(dy.shape[:2], dtype=t.bool)
    for z, s in zip(zs, sums):
        ambiguous |= (z.abs() <= 1e-5 * s).any(-1)
    dy[ambiguous] = 0.0
    return x, ws, bs, dy, float(ambiguous.float().mean())


def errors(got, ref):
    return [float((g.detach().cpu().double() - r).abs().max()
                  / r.abs().max().clamp_min(1e-300))
            for g, r in zip(got, ref)]


def same_bits(a, b):
    return all(t.equal(u.view(t.uint8), v.view(t.uint8))
               for u, v in zip(a, b))


@cases
def test_exact_on_sparse_integers(case):
    x, ws, bs, dy = exact_inputs(case)
    ref, zs, _ = reference(x, ws, bs, dy)
    bound, hidden, _ = reference(x.abs(), [w.abs() for w in ws],
                                 [b.abs() for b in bs], dy.abs(),
                                 absolute=True)
    assert max(float(v.max()) for v in bound + hidden) < 2 ** 24
    assert any(bool((z == 0).any()) for z in zs)
    got = run(ops.fused_mlp, case, x, ws, bs, dy)
    for name, g, r in zip(["y", "dx"] + ["dW"] * len(ws) + ["db"] * len(ws),
                          got, ref):
        assert g.shape == r.shape, name
        assert t.equal(g.cpu().double(), r), name


@cases
def test_general_inputs(case):
    x, ws, bs, dy, ambiguous = general_inputs(case)
    assert ambiguous <= 0.02
    ref, _, _ = reference(x, ws, bs, dy)
    kernel = errors(run(ops.fused_mlp, case, x, ws, bs, dy), ref)
    torch_form = errors(run(ops._fused_mlp_torch, case, x, ws, bs, dy), ref)
    print(f"{CASES[case]}: kernel / torch-form error "
          + " ".join(f"{k:.2e}/{f:.2e}" for k, f in zip(kernel, torch_form)))
    for k, f in zip(kernel, torch_form):
        assert k <= 4 * f + 2.0 ** -22


@cases
def test_same_bits(case):
    x, ws, bs, dy, _ = general_inputs(case)
    got = run(ops.fused_mlp, case, x, ws, bs, dy)
    assert same_bits(got, run(ops.fused_mlp, case, x, ws, bs, dy))
    frozen = run(ops.fused_mlp, case, x, ws, bs, dy, need_x=False)
    assert frozen[1] is None
    assert same_bits(got[:1] + got[2:], frozen[:1] + frozen[2:])
    with t.no_grad():
        dev = [v.float().to(DEV) for v in [x] + ws + bs]
        E, _, _, shared = CASES[case]
        if E is None or shared:
            dev[0] = dev[0][0]
        if E is None:
            dev[1:] = [v[0] for v in dev[1:]]
        y = ops.fused_mlp(dev[0], dev[1:1 + len(ws)], dev[1 + len(ws):])
    assert same_bits([y if E is not None else y[None]], got[:1])


def test_above_the_batch_limit_runs_the_torch_form(monkeypatch):
    x, ws, bs, dy, _ = general_inputs(3)   # B = 5
    monkeypatch.setattr(ops, "FUSED_MLP_MAX_BATCH", 4)
    routed = run(ops.fused_mlp, 3, x, ws, bs, dy)
    assert same_bits(routed, run(ops._fused_mlp_torch, 3, x, ws, bs, dy))


def test_fused_mlp_module_takes_an_sgd_step(monkeypatch):
    E, B, sizes, _ = CASES[1]
    x, ws, bs, dy, _ = general_inputs(1)
    ref, _, _ = reference(x, ws, bs, dy)
    want = [p[0] - 0.1 * g[0] for p, g in zip(ws + bs, ref[2:])]

    def step():
        net = FusedMLP(sizes)
        with t.no_grad():
            for p, v in zip(list(net.weights) + list(net.biases), ws + bs):
                p.copy_(v[0])
        net = net.to(DEV)
        opt = t.optim.SGD(net.parameters(), lr=0.1)
        (net(x[0].float().to(DEV)) * dy[0].float().to(DEV)).sum().backward()
        opt.step()
        return list(net.weights) + list(net.biases)

    kernel = errors(step(), want)
    monkeypatch.setattr(ops, "FUSED_MLP_MAX_BATCH", 0)
    torch_form = errors(step(), want)
    for k, f in zip(kernel, torch_form):
        assert k <= 4 * f + 2.0 ** -22
