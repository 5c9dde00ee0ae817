"""``ConvBiasReLU2d(impl=...)`` where the implicit-GEMM kernels do not
apply: the call takes the library path, bit for bit; and the share of
outputs near the ReLU's kink in the GPU test's reference."""
import pytest
import torch as t

from machin_amd.ops.fused_conv import ConvBiasReLU2d
from util_conv_igemm import CASES, case_id, reference

DEVICES = ["cpu"] + (["cuda:0"] if t.cuda.is_available() else [])
# what makes the call ineligible: (kernel size, dtype, channels-last x)
INELIGIBLE = {"fp32": (4, t.float32, True), "nchw": (4, t.bfloat16, False),
              "geometry": (5, t.bfloat16, True)}


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("why", INELIGIBLE)
def test_ineligible_calls_take_the_library_path(device, why):
    k, dtype, channels_last = INELIGIBLE[why]
    t.manual_seed(0)
    hip = ConvBiasReLU2d(32, 64, k, stride=2, impl="hip")
    ref = ConvBiasReLU2d(32, 64, k, stride=2, impl="miopen")
    ref.load_state_dict(hip.state_dict())
    x = t.randn(2, 32, 8, 8).to(device, dtype)
    if channels_last:
        x = x.contiguous(memory_format=t.channels_last)
    results = []
    for mod in (hip.to(device, dtype), ref.to(device, dtype)):
        xi = x.clone().requires_grad_()
        y = mod(xi)
        y.backward(t.ones_like(y))
        results.append([y, xi.grad, mod.weight.grad, mod.bias.grad])
    for got, want in zip(*results):
        assert t.equal(got, want)


def test_unknown_impl_raises(monkeypatch):
    with pytest.raises(ValueError):
        ConvBiasReLU2d(32, 64, 4, stride=2, impl="cudnn")
    monkeypatch.setenv("MACHIN_CONV_IMPL", "cudnn")
    with pytest.raises(ValueError):
        ConvBiasReLU2d(32, 64, 4, stride=2)(t.zeros(1, 32, 4, 4))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_reference_rarely_sits_on_the_relu_kink(case):
    # the GPU test leaves the side of the ReLU open at these elements
    r = reference(case, "normal")
    assert (r.s.abs() <= r.bound).double().mean().item() < 0.02
