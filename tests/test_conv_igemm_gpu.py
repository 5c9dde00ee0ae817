"""The implicit-GEMM conv2/conv3 kernels (``ConvBiasReLU2d(impl="hip")``)
against ``F.conv2d`` and its autograd in float64 on the CPU, on the
bf16-rounded inputs.

Bound on general inputs. The kernels multiply bf16 operands exactly
into fp32, add the K = KH*KW*Cin products in fp32 in some order and
round the sum once to bf16. A sum of K terms accumulated in fp32 in
any order is within (K - 1) * 2^-24 * sum|terms| of the exact sum (each
of the K - 1 additions rounds a partial sum no larger than sum|terms|);
adding the fp32 bias is one more such step, and the rounding to bf16
(8 significand bits, round to nearest) is within 2^-9 of the value.
With sum|terms| = conv(|x|, |w|) and ref = relu(s):

    |y - ref| <= 2^-8 |ref| + K * 2^-23 * conv(|x|, |w|)

which leaves a factor two on both parts (the second also covers the
bias step and the first-order cross term). An output whose float64
pre-activation s lies within the bound of zero may be clamped on one
side of the comparison and kept on the other; those elements are left
out, and required to be under 2% (test_conv_igemm_cpu.py checks that
share on the reference alone). There the backward mask may differ too,
so the gradient reference takes the ReLU's derivative where the
kernel's activation is positive. dx is the same kind of sum over its
(KH/S)^2 * Cout terms per parity class, rounded once, with the masked
bf16 gradient as operand:

    |dx - ref| <= 2^-8 |ref| + (KH/S)^2 Cout * 2^-23 * conv_T(|g|, |w|)

On integer inputs (ranges in util_conv_igemm.reference) every fp32 sum
is exact, so y and dx equal the float64 result rounded once to bf16."""
import pytest
import torch as t

pytestmark = pytest.mark.gpu

if not t.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from machin_amd.model.nets.nature_cnn import FusedActorCriticCNN  # noqa: E402
from machin_amd.ops.fused_conv import ConvBiasReLU2d  # noqa: E402
from util_conv_igemm import (  # noqa: E402
    CASES, GEOMETRY, backward_reference, case_id, reference,
)

DEV = "cuda:0"


def _run(case, kind, monkeypatch, autocast=False):
    """bf16 y [N, Cout, OH, OW] and dx, and dW, db, of the module on the
    case's inputs, on the CPU. Without autocast the module is bf16 and
    its parameters take no gradient (dW is the library's)."""
    geom, _, _, _, flat, wg = case
    cin, cout, k, stride = GEOMETRY[geom]
    if wg is None:
        monkeypatch.delenv("MACHIN_CONV_IGEMM_WG", raising=False)
    else:
        monkeypatch.setenv("MACHIN_CONV_IGEMM_WG", str(wg))
    r = reference(case, kind)
    conv = ConvBiasReLU2d(cin, cout, k, stride=stride, flatten=flat,
                          impl="hip").to(DEV)
    with t.no_grad():
        conv.weight.copy_(r.w)
        conv.bias.copy_(r.b)
    if not autocast:
        conv = conv.to(t.bfloat16).requires_grad_(False)
    xd = r.x.to(DEV, t.bfloat16).contiguous(
        memory_format=t.channels_last).requires_grad_()
    gyd = r.gy.to(DEV, t.bfloat16)
    with t.autocast("cuda", dtype=t.bfloat16, enabled=autocast):
        y = conv(xd)
    assert "Igemm" in type(y.grad_fn).__name__  # no fallback
    y.backward(gyd.flatten(1) if flat else gyd)
    return tuple(None if v is None else v.detach().cpu().contiguous()
                 for v in (y.view(r.gy.shape), xd.grad, conv.weight.grad,
                           conv.bias.grad))


def _same_bits(a, b):
    return t.equal(a.view(t.int16), b.view(t.int16))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_exact_on_integers(case, monkeypatch):
    y, dx, _, _ = _run(case, "integer", monkeypatch)
    r = reference(case, "integer")
    # "+ 0.0": an exact zero sum is +0, as the ReLU's zero is
    y_ref = (r.s.clamp_min(0.0) + 0.0).to(t.bfloat16)
    assert _same_bits(y, y_ref)
    dx_ref = backward_reference(case, "integer", y_ref > 0)[0] + 0.0
    assert _same_bits(dx, dx_ref.to(t.bfloat16))
    # rows and columns that no tap reaches: exact zeros
    reach = [(n - 1) * r.stride + r.k for n in r.gy.shape[2:]]
    assert not dx[:, :, reach[0]:].any() and not dx[:, :, :, reach[1]:].any()
    if case == ("conv2", 3, 7, 9, False, None):
        assert reach[0] == 6 and dx.shape[2] == 7  # row 6 is such a row
    y2, dx2, _, _ = _run(case, "integer", monkeypatch)
    assert _same_bits(y, y2) and _same_bits(dx, dx2)


def _check_general(case, got):
    y, dx = got[0].double(), got[1].double()
    r = reference(case, "normal")
    open_side = r.s.abs() <= r.bound
    excess = ((y - r.s.clamp_min(0.0)).abs() - r.bound)[~open_side].max()
    dx_ref, dw_ref, db_ref, abs_sum = backward_reference(
        case, "normal", y > 0)
    terms = (r.k // r.stride) ** 2 * r.cout
    dx_bound = 2.0 ** -8 * dx_ref.abs() + terms * 2.0 ** -23 * abs_sum
    dx_excess = ((dx - dx_ref).abs() - dx_bound).max()
    print(f"{case_id(case)}: open share {open_side.double().mean():.4f}, "
          f"excess over the bound y {excess:.3e}, dx {dx_excess:.3e}")
    assert open_side.double().mean() < 0.02
    assert (y == 0).double().mean() > 0.3  # a good share is clamped
    assert excess <= 0.0 and dx_excess <= 0.0
    return dw_ref, db_ref


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_general_inputs_within_derived_bound(case, monkeypatch):
    _check_general(case, _run(case, "normal", monkeypatch))


@pytest.mark.parametrize(
    "case", [("conv2", 5, 20, 20, False, None),
             ("conv3", 5, 9, 9, True, None)], ids=case_id)
def test_module_end_to_end(case, monkeypatch):
    got = _run(case, "normal", monkeypatch, autocast=True)
    dw_ref, db_ref = _check_general(case, got)
    # the bias gradient is summed in fp32 and rounded to bf16: one step
    step = t.pow(2.0, t.floor(t.log2(db_ref.abs().clamp_min(2.0 ** -126))) - 7)
    assert ((got[3] - db_ref).abs() <= step).all()
    assert (got[2] - dw_ref).abs().max() <= 2.0 ** -8 * dw_ref.abs().max()


def test_model_with_hip_convs():
    default = FusedActorCriticCNN().to(DEV)
    model = FusedActorCriticCNN(conv_impl="hip").to(DEV).to(
        memory_format=t.channels_last)
    model.load_state_dict(default.state_dict())
    frames = t.randint(0, 256, (3, 4, 84, 84), dtype=t.uint8, device=DEV)
    frames = frames.contiguous(memory_format=t.channels_last)
    with t.autocast("cuda", dtype=t.bfloat16):
        h = model.stem(frames)
        for layer in (model.conv_rest[0], model.conv_rest[2]):
            h = layer(h)  # conv_impl reached both layers: no fallback
            assert "Igemm" in type(h.grad_fn).__name__
    logits, value = model(frames)
    (logits.float().square().mean() + value.float().square().mean()).backward()
    for name, p in model.named_parameters():
        assert p.grad is not None and t.isfinite(p.grad).all(), name
