"""The hand-written conv2/conv3 weight gradient (``ext.conv_igemm_wrw``,
``ConvBiasReLU2d(impl="hip_wrw")``) against float64 autograd on the CPU.

Bound on general inputs, as derived in test_conv_igemm_gpu.py: bf16
products are exact in fp32, the R = N*OH*OW terms of an element are added
in fp32 in some order (the slab sums included) and the sum is rounded
once to bf16, so with A = the weight gradient of (|x|, |g|)

    |dW - ref| <= 2^-8 |ref| + R * 2^-23 * A

On integer inputs every fp32 sum is exact and dW equals the float64
result rounded once to bf16 ("+ 0.0": an exact zero sum is +0)."""
import pytest
import torch as t

pytestmark = pytest.mark.gpu

if not t.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import util_conv_igemm  # noqa: E402
from machin_amd.model.nets.nature_cnn import FusedActorCriticCNN  # noqa: E402
from machin_amd.ops import _require_ext  # noqa: E402
from machin_amd.ops.fused_conv import ConvBiasReLU2d  # noqa: E402
from util_conv_igemm import (  # noqa: E402
    GEOMETRY, backward_reference, case_id, reference,
)

DEV = "cuda:0"
# (geometry, N, H, W, flatten, MACHIN_CONV_IGEMM_WG or None)
CASES = [(geom, n, h, w, False, wg) for geom, shapes in (
    ("conv2", ((1, 4, 4, 2), (3, 7, 9, 2), (5, 20, 20, 2), (203, 4, 4, 2),
               (67, 20, 20, None))),
    ("conv3", ((1, 3, 3, 2), (3, 5, 4, 2), (5, 9, 9, 2), (203, 3, 3, 2),
               (67, 9, 9, None))),
) for n, h, w, wg in shapes]


@pytest.fixture
def case(request, monkeypatch):
    """The case, known to ``reference`` (which seeds by the position in
    its list) and with the case's grid in the environment."""
    case = request.param
    if case not in util_conv_igemm.CASES:
        monkeypatch.setattr(util_conv_igemm, "CASES",
                            util_conv_igemm.CASES + [case])
    if case[5] is None:
        monkeypatch.delenv("MACHIN_CONV_IGEMM_WG", raising=False)
    else:
        monkeypatch.setenv("MACHIN_CONV_IGEMM_WG", str(case[5]))
    return case


def _nhwc(v):
    return v.to(DEV, t.bfloat16).permute(0, 2, 3, 1).contiguous()


def _wrw(case, kind):
    r = reference(case, kind)
    return _require_ext().conv_igemm_wrw(
        _nhwc(r.gy), _nhwc(r.x), r.k, r.stride).cpu()


def _excess(case, dw, dw_ref, g_abs):
    """Largest excess of |dW - ref| over the derived bound."""
    r = reference(case, "normal")
    x, w = r.x.abs(), r.w.clone().requires_grad_()
    (a,) = t.autograd.grad(
        t.nn.functional.conv2d(x, w, None, r.stride), w, g_abs)
    terms = g_abs.numel() // r.cout
    bound = 2.0 ** -8 * dw_ref.abs() + terms * 2.0 ** -23 * a
    return ((dw.double() - dw_ref).abs() - bound).max().item()


@pytest.mark.parametrize("case", CASES, ids=case_id, indirect=True)
def test_exact_on_integers(case):
    r = reference(case, "integer")
    ones = t.ones_like(r.gy, dtype=t.bool)
    dw_ref = (backward_reference(case, "integer", ones)[1] + 0.0).bfloat16()
    dw = _wrw(case, "integer")
    assert dw.shape == r.w.shape
    assert t.equal(dw.view(t.int16), dw_ref.view(t.int16))
    assert t.equal(_wrw(case, "integer").view(t.int16), dw.view(t.int16))


@pytest.mark.parametrize("case", CASES, ids=case_id, indirect=True)
def test_general_inputs_within_derived_bound(case):
    r = reference(case, "normal")
    ones = t.ones_like(r.gy, dtype=t.bool)
    dw_ref = backward_reference(case, "normal", ones)[1]
    excess = _excess(case, _wrw(case, "normal"), dw_ref, r.gy.abs())
    print(f"{case_id(case)}: excess over the bound dW {excess:.3e}")
    assert excess <= 0.0


@pytest.mark.parametrize("case", [("conv2", 5, 20, 20, True, None),
                                  ("conv3", 5, 9, 9, True, None)],
                         ids=case_id, indirect=True)
def test_through_the_module(case):
    cin, cout, k, stride = GEOMETRY[case[0]]
    r = reference(case, "normal")
    got = {}
    for impl in ("hip_wrw", "hip"):
        conv = ConvBiasReLU2d(cin, cout, k, stride=stride, flatten=True,
                              impl=impl).to(DEV)
        with t.no_grad():
            conv.weight.copy_(r.w)
            conv.bias.copy_(r.b)
        x = r.x.to(DEV, t.bfloat16).contiguous(
            memory_format=t.channels_last).requires_grad_()
        with t.autocast("cuda", dtype=t.bfloat16):
            y = conv(x)
        got[impl + "_fn"] = type(y.grad_fn).__name__
        y.backward(r.gy.to(DEV, t.bfloat16).flatten(1))
        got[impl] = [v.detach().cpu() for v in (y, x.grad, conv.weight.grad)]
    assert "IgemmWrw" in got["hip_wrw_fn"]  # no fallback
    assert "IgemmWrw" not in got["hip_fn"]
    y, dx, dw = got["hip_wrw"]
    assert t.equal(y.view(t.int16), got["hip"][0].view(t.int16))
    assert t.equal(dx.view(t.int16), got["hip"][1].view(t.int16))
    mask = y.view(r.gy.shape) > 0
    dw_ref = backward_reference(case, "normal", mask)[1]
    excess = _excess(case, dw, dw_ref, t.where(mask, r.gy, 0.0).abs())
    print(f"{case_id(case)}: excess over the bound dW {excess:.3e}")
    assert excess <= 0.0


def test_model_with_hip_wrw_convs():
    model = FusedActorCriticCNN(conv_impl="hip_wrw").to(DEV).to(
        memory_format=t.channels_last)
    frames = t.randint(0, 256, (3, 4, 84, 84), dtype=t.uint8, device=DEV)
    frames = frames.contiguous(memory_format=t.channels_last)
    with t.autocast("cuda", dtype=t.bfloat16):
        h = model.stem(frames)
        for layer in (model.conv_rest[0], model.conv_rest[2]):
            h = layer(h)
            assert "IgemmWrw" in type(h.grad_fn).__name__
    logits, value = model(frames)
    (logits.float().square().mean() + value.float().square().mean()).backward()
    for name, p in model.named_parameters():
        assert p.grad is not None and t.isfinite(p.grad).all(), name
